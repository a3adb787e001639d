"""The gather's second wire format (rpt_gather_set_moments; csrc/k_gather.h) without a GPU: the layout arithmetic (rpt_debug_gather_layout) and the host build
of pack -> slots -> un-tile (rpt_debug_gather_host) against a numpy restatement built from rpt_tile_order alone.  The kernels and comm_configure run the
same RPT_HD functions; tests/test_gpu_gather_moments.py holds them to the single context's records on the device."""
import numpy as np
import pytest

SIZES = [(100, 70), (130, 67)]          # four tiles, three of them clipped; six tiles
WORLDS = [1, 2, 3, 5, 8]


def _orders(hipmod, W, H, world):
    return [hipmod.tile_order(W, H, r, world) for r in range(world)]


def _index(order, W):
    return (order >> 16).astype(np.int64) * W + (order & 0xFFFF).astype(np.int64)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("world", WORLDS)
def test_layout_is_the_restatement(hipmod, W, H, world):
    """stride = the largest block; a slot = two strides of records and one trailer record; every rank's message is its whole slot"""
    orders = _orders(hipmod, W, H, world)
    blocks = [len(o) for o in orders]
    assert sum(blocks) == W * H
    stride = max(blocks)
    lay = hipmod.gather_layout(W, H, world, True)
    assert lay["stride"] == stride and lay["block_pixels"] == blocks
    assert lay["slot_floats"] == (2 * stride + 1) * 4
    assert lay["message_floats"] == [(2 * stride + 1) * 4] * world


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("world", WORLDS)
def test_plain_layout_is_todays(hipmod, W, H, world):
    """with_moments = 0: what comm_configure computes for the plain gather — the stride is the largest block, a rank sends its block and nothing else, a rank
    that owns nothing posts nothing"""
    blocks = [len(o) for o in _orders(hipmod, W, H, world)]
    lay = hipmod.gather_layout(W, H, world, False)
    assert lay["stride"] == max(blocks) and lay["slot_floats"] == max(blocks) * 4
    assert lay["block_pixels"] == blocks and lay["message_floats"] == [4 * b for b in blocks]


def test_the_cases_exercise_the_padding(hipmod):
    """100 x 70 has four tiles: over five ranks one rank owns nothing, over three ranks the three blocks differ (two tiles, one, one — all clipped differently)"""
    assert 0 in hipmod.gather_layout(100, 70, 5)["block_pixels"]
    b = hipmod.gather_layout(100, 70, 3)["block_pixels"]
    assert len(set(b)) == 3 and min(b) > 0


def _hostile(rng, n):
    """records of NaN, +-inf, denormals, 0xffffffff and ordinary values, as bit patterns"""
    special = np.array([0x7FC00000, 0x7F800001, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0xFFFFFFFF, 0x00000000, 0x80000000], np.uint32)
    bits = rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    pick = rng.random((n, 4)) < 0.5
    bits[pick] = special[rng.integers(0, len(special), size=int(pick.sum()))]
    return bits


SENTINEL = 0xDEADBEEF


def _expected(hipmod, W, H, world, accum_bits, moments_bits, trailers):
    """the slots and the two images in numpy, from rpt_tile_order"""
    orders = _orders(hipmod, W, H, world)
    stride = max(len(o) for o in orders)
    slot = 2 * stride + 1
    slots = np.full((world, slot, 4), SENTINEL, np.uint32)
    image, moments = np.zeros((H * W, 4), np.uint32), np.zeros((H * W, 4), np.uint32)
    first = 0
    for r, o in enumerate(orders):
        n = len(o)
        slots[r, :n] = accum_bits[first:first + n]
        slots[r, stride:stride + n] = moments_bits[first:first + n]
        slots[r, 2 * stride] = trailers[r]
        image[_index(o, W)] = accum_bits[first:first + n]
        moments[_index(o, W)] = moments_bits[first:first + n]
        first += n
    return slots, image.reshape(H, W, 4), moments.reshape(H, W, 4)


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("world", WORLDS)
def test_host_gather_moves_every_word(hipmod, W, H, world):
    """both images word for word on hostile records; the padding of the landing buffer keeps the caller's sentinel (never written) and the sentinel reaches
    neither image"""
    rng = np.random.default_rng(1000 * world + W)
    accum_bits, moments_bits = _hostile(rng, W * H), _hostile(rng, W * H)
    assert not (accum_bits == SENTINEL).any() and not (moments_bits == SENTINEL).any()
    blocks = hipmod.gather_layout(W, H, world)["block_pixels"]
    trailers = np.array([[hipmod.GATHER_FORMAT, 0, 8, b] for b in blocks], np.uint32)
    want_slots, want_image, want_moments = _expected(hipmod, W, H, world, accum_bits, moments_bits, trailers)
    slots = np.full(want_slots.size, SENTINEL, np.uint32).view(np.float32)
    image, moments, info = hipmod.gather_host(W, H, world, accum_bits.view(np.float32), moments_bits.view(np.float32), trailers, slots)
    assert np.array_equal(slots.view(np.uint32).reshape(want_slots.shape), want_slots)
    assert np.array_equal(image.view(np.uint32), want_image) and np.array_equal(moments.view(np.uint32), want_moments)
    assert not (image.view(np.uint32) == SENTINEL).any() and not (moments.view(np.uint32) == SENTINEL).any()
    assert info == {"with_moments": 1, "nonuniform": 0, "samples_min": 8, "samples_max": 8, "bad_trailers": 0}
    # without a landing buffer of the caller's: a zeroed one, the same images
    image2, moments2, info2 = hipmod.gather_host(W, H, world, accum_bits.view(np.float32), moments_bits.view(np.float32), trailers)
    assert np.array_equal(image2.view(np.uint32), want_image) and np.array_equal(moments2.view(np.uint32), want_moments) and info2 == info


def test_info_words_from_the_trailers(hipmod):
    """trailers that agree, that differ in the sample count, that carry one non-uniform flag, one bad format word; a rank without pixels says nothing about the
    image; the result does not depend on the order of the ranks' trailers"""
    W, H, world = 100, 70, 5
    blocks = hipmod.gather_layout(W, H, world)["block_pixels"]
    empty = blocks.index(0)
    zeros = np.zeros((W * H, 4), np.float32)
    F = hipmod.GATHER_FORMAT

    def info(rows):
        return hipmod.gather_host(W, H, world, zeros, zeros, np.array(rows, np.uint32))[2]

    agree = [[F, 0, 12, b] for b in blocks]
    assert info(agree) == {"with_moments": 1, "nonuniform": 0, "samples_min": 12, "samples_max": 12, "bad_trailers": 0}
    for r in [k for k in range(world) if k != empty]:
        rows = [list(t) for t in agree]
        rows[r][2] = 4                                   # one rank rendered fewer uniform samples: every pixel by its own count
        assert info(rows) == {"with_moments": 1, "nonuniform": 1, "samples_min": 4, "samples_max": 12, "bad_trailers": 0}
        rows = [list(t) for t in agree]
        rows[r][1] = 1                                   # one rank's masked pass
        assert info(rows) == {"with_moments": 1, "nonuniform": 1, "samples_min": 12, "samples_max": 12, "bad_trailers": 0}
        rows = [list(t) for t in agree]
        rows[r][0] = 0                                   # a rank on the plain format: its slot's last record is not a trailer
        got = info(rows)
        assert got["bad_trailers"] == 1 and got["with_moments"] == 1
    rows = [list(t) for t in agree]
    rows[empty][1:3] = [1, 99]                           # the rank that owns nothing
    assert info(rows) == info(agree)
    rows[empty][0] = 0xFFFFFFFF
    assert info(rows)["bad_trailers"] == 1
    # world 1, and a refusal
    one = hipmod.gather_host(64, 64, 1, np.zeros((4096, 4), np.float32), np.zeros((4096, 4), np.float32), np.array([[F, 1, 3, 4096]], np.uint32))[2]
    assert one == {"with_moments": 1, "nonuniform": 1, "samples_min": 3, "samples_max": 3, "bad_trailers": 0}
    with pytest.raises(hipmod.RptError):
        hipmod.gather_layout(0, 70, 2)
    with pytest.raises(hipmod.RptError):
        hipmod.gather_layout(100, 70, 65)
