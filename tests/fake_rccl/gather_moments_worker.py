"""One RANK of a multi-process render whose gather carries the moments record and the counts flag (rpt_gather_set_moments), through the C ABI:

    rpt_create -> rpt_comm_init -> rpt_upload_scene / rpt_set_config -> rpt_set_moments -> rpt_gather_set_moments(1) -> rpt_reset
    every rank:  rpt_render_async(n) ; rpt_gather_async
    ONLY --masked-rank:  rpt_render_pixels(mask, n)          (the ranks are masked differently: the root's own counts stay uniform)
    every rank:  rpt_gather_async
    rank 0:      rpt_read_gathered, rpt_read_gathered_moments, rpt_gathered_info_get, rpt_counts_uniform, rpt_denoise_variance(RPT_DENOISE_GATHERED, NULL)

Started by tests/test_gpu_gather_moments_processes.py with RPT_RCCL_LIBRARY pointing at tests/fake_rccl/librccl_fake.so, every rank on the one GPU of the test
box.  Rank 0 writes <out>/root.json and the arrays beside it; every rank writes <out>/rank<r>.json."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--uid", required=True)
    ap.add_argument("--rank", type=int, required=True)
    ap.add_argument("--world", type=int, required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--scene", default="DarkCornell")
    ap.add_argument("--width", type=int, required=True)
    ap.add_argument("--height", type=int, required=True)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--masked-rank", type=int, required=True)
    ap.add_argument("--mask", required=True, help="x0,y0,x1,y1: the rectangle the masked rank renders again")
    args = ap.parse_args()

    rpt = importlib.import_module("rust-path-tracer_amd")
    hip = importlib.import_module("rust-path-tracer_amd.hip")
    cfg = rpt.default_config(args.width, args.height, nee=1)
    x0, y0, x1, y1 = (int(v) for v in args.mask.split(","))
    mask = np.zeros((args.height, args.width), np.uint8)
    mask[y0:y1, x0:x1] = 1

    r = hip.Renderer(0, rank=args.rank, world_size=args.world)
    r.comm_init(bytes.fromhex(args.uid), args.rank, args.world)
    r.upload_scene(rpt.World.from_path(rpt.fixture(args.scene + ".glb")))
    r.set_config(cfg)
    r.set_moments(True)
    r.gather_set_moments(True)
    r.reset(rpt.blue_noise_seeds(args.width, args.height))
    r.render_async(args.samples)
    r.gather_async()
    if args.rank == args.masked_rank:
        r.render_pixels(mask, args.samples)
    r.gather_async()
    r.gather_wait()
    r.wait()
    info = {"rank": args.rank, "pixels": int(r.local_pixels()), "counts_uniform": bool(r.counts_uniform()), "gather_moments": bool(r.gather_moments())}
    if args.rank == 0:
        img, samples = r.read_gathered()
        np.save(os.path.join(args.out, "image.npy"), img)
        np.save(os.path.join(args.out, "moments.npy"), r.read_gathered_moments())
        rgb, var = r.denoise_variance(source=hip.DENOISE_GATHERED, moments=None, params=hip.denoise_var_params(iterations=3, sigma_variance=4.0), tonemap_op=3)
        np.save(os.path.join(args.out, "denoised.npy"), rgb)
        np.save(os.path.join(args.out, "variance.npy"), var)
        info.update(gathered_samples=int(samples), gathered_info=r.gathered_info())
    with open(os.path.join(args.out, f"rank{args.rank}.json"), "w") as f:
        json.dump(info, f)
    r.close()


if __name__ == "__main__":
    main()
