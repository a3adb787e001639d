"""Renderer: ctypes over the rpt.h C ABI of librpt_hip.so (the MI355X wavefront path tracer).

Every method maps 1:1 to a C entry point, which in turn cites the reference
call it replaces (include/rpt/rpt.h; reference: src/trace.rs:136-224).
There is deliberately NO fallback: if the HIP library is missing or no GPU is
present this module raises.
"""
import ctypes as C
import os

import numpy as np

from . import _ffi
from ._ffi import MATERIAL_MODEL_DTYPE, MATERIAL_VOLUME_DTYPE, PUNCTUAL_LIGHT_DTYPE, RNG_DTYPE, Stats, TracingConfig, ptr

_lib = None

COMM_ID_BYTES = 128
SHADOW_EXACT, SHADOW_SEGMENT = 0, 1          # rpt_set_shadow_mode
WALK_NEAREST_PLAIN, WALK_NEAREST_FIRST, WALK_NEAREST_LAST, WALK_SHADOW = 0, 1, 2, 3       # rpt_debug_walk_production
MODEL_PBR, MODEL_LAMBERTIAN, MODEL_GLASS = 0, 1, 2      # rpt_set_material_models


def material_models(models, iors=None):
    """records for set_material_models: one MODEL_* per material, and the ior of the GLASS ones (a scalar or one per material; default 1.5)"""
    rec = np.zeros(len(models), MATERIAL_MODEL_DTYPE)
    rec["model"] = models
    rec["ior"] = 1.5 if iors is None else iors
    return rec


def material_volumes(sigmas):
    """records for set_material_volumes: one (r, g, b) absorption per unit scene length per material (zeros: the material does not absorb)"""
    sigmas = np.asarray(sigmas, np.float32).reshape(-1, 3)
    rec = np.zeros(len(sigmas), MATERIAL_VOLUME_DTYPE)
    rec["sigma"] = sigmas
    return rec


def absorption(color, distance):
    """sigma of glTF's KHR_materials_volume: the (r, g, b) absorption under which white light has `color` after `distance` scene units,
    -ln(color) / distance in float64, rounded to float32; colour channels are clamped to [0, 1], a channel of 0 gives the largest finite float"""
    color = np.clip(np.asarray(color, np.float64), 0.0, 1.0)
    if not (np.isfinite(distance) and distance > 0):
        raise ValueError("absorption: the distance must be finite and above 0")
    with np.errstate(divide="ignore"):
        sigma = -np.log(color) / float(distance)
    fmax = float(np.finfo(np.float32).max)
    return np.where(color == 0.0, fmax, np.minimum(sigma, fmax)).astype(np.float32) + np.float32(0.0)      # (+ 0: -0.0 of a channel of 1 becomes +0.0)


LIGHT_POINT, LIGHT_SPOT, LIGHT_DIRECTIONAL = 0, 1, 2      # rpt_set_punctual_lights


def _light(kind, position=(0.0, 0.0, 0.0), direction=None, intensity=(1.0, 1.0, 1.0), scale=0.0, offset=0.0):
    rec = np.zeros(1, PUNCTUAL_LIGHT_DTYPE)
    rec["type"] = kind
    rec["position"] = np.asarray(position, np.float64)
    if direction is not None:
        d = np.asarray(direction, np.float64)
        length = float(np.sqrt(np.sum(d * d)))
        if not (np.isfinite(length) and length > 0):
            raise ValueError("a light's direction must be finite and not zero")
        rec["direction"] = d / length               # normalised in float64, rounded once
    rec["intensity"] = np.broadcast_to(np.asarray(intensity, np.float64), (3,))
    rec["angle_scale"], rec["angle_offset"] = scale, offset
    return rec


def point_light(position, intensity):
    """one record for set_punctual_lights: a point light of radiant intensity (r, g, b) per steradian (a scalar: white)"""
    return _light(LIGHT_POINT, position, None, intensity)


def spot_light(position, direction, intensity, inner_deg, outer_deg):
    """one record for set_punctual_lights: a spot light shining along `direction` (normalised here), full inside the inner cone angle, nothing outside the
    outer one, glTF's smooth step between: angle_scale = 1 / max(0.001, cos inner - cos outer), angle_offset = -cos outer * angle_scale (float64, rounded once)"""
    ci, co = np.cos(np.radians(float(inner_deg))), np.cos(np.radians(float(outer_deg)))
    scale = 1.0 / max(0.001, ci - co)
    return _light(LIGHT_SPOT, position, direction, intensity, scale, -co * scale)


def directional_light(direction, irradiance):
    """one record for set_punctual_lights: a directional light shining along `direction` (normalised here) with irradiance (r, g, b) on a surface facing it"""
    return _light(LIGHT_DIRECTIONAL, (0.0, 0.0, 0.0), direction, irradiance)


def punctual_lights(*records):
    """the records of point_light / spot_light / directional_light (or arrays of PUNCTUAL_LIGHT_DTYPE) joined into one array"""
    if not records:
        return np.zeros(0, PUNCTUAL_LIGHT_DTYPE)
    return np.concatenate([np.ascontiguousarray(r, PUNCTUAL_LIGHT_DTYPE).reshape(-1) for r in records])


class CameraLens(C.Structure):
    """rpt_camera_lens"""
    _fields_ = [("tan_half_fov", C.c_float), ("aperture_radius", C.c_float), ("focus_distance", C.c_float), ("reserved", C.c_uint32)]


def tan_half_fov(degrees):
    """tan_half_fov of a HORIZONTAL field of view in degrees (90: the reference's camera, 1.0)"""
    import math
    return 1.0 if degrees == 90 else math.tan(math.radians(degrees) / 2.0)


def camera_lens(tan_half_fov=1.0, aperture_radius=0.0, focus_distance=1.0):
    """an rpt_camera_lens; the defaults are the reference's pinhole"""
    return CameraLens(tan_half_fov, aperture_radius, focus_distance, 0)


MULTI_ALLOW_SHARED_DEVICE = 1
DENOISE_ACCUM, DENOISE_GATHERED = 0, 1       # rpt_denoise: which image
GUIDE_MISS, GUIDE_SURFACE, GUIDE_EMITTER = 0, 1, 2


class DenoiseParams(C.Structure):
    """rpt_denoise_params (include/rpt/rpt.h)"""
    _fields_ = [("iterations", C.c_uint32), ("normal_power_log2", C.c_uint32), ("sigma_color", C.c_float), ("sigma_plane", C.c_float),
                ("demodulate", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class DenoiseVarParams(C.Structure):
    """rpt_denoise_var_params"""
    _fields_ = [("base", DenoiseParams), ("sigma_variance", C.c_float), ("clamp_scale", C.c_float), ("clamp_floor", C.c_float), ("clamp_radius", C.c_uint32)]


class DenoiseReport(C.Structure):
    """rpt_denoise_report"""
    _fields_ = [("device_ms", C.c_double), ("guides_ms", C.c_double), ("guides_rebuilt", C.c_uint32), ("pixels_clamped", C.c_uint32)]


class TemporalParams(C.Structure):
    """rpt_temporal_params"""
    _fields_ = [("filter", DenoiseVarParams), ("max_history", C.c_float), ("normal_min", C.c_float), ("plane_max", C.c_float), ("reserved", C.c_uint32 * 5)]


class TemporalReport(C.Structure):
    """rpt_temporal_report"""
    _fields_ = [("base", DenoiseReport), ("pixels_with_history", C.c_uint64), ("history_state", C.c_uint32), ("reserved", C.c_uint32)]


HISTORY_NONE, HISTORY_USED, HISTORY_DROPPED = 0, 1, 2      # rpt_temporal_report.history_state


class NoiseCounts(C.Structure):
    """rpt_noise_counts"""
    _fields_ = [("pixels", C.c_uint64), ("measured", C.c_uint64), ("above", C.c_uint64)]


class NoiseTarget(C.Structure):
    """rpt_noise_target"""
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_uint32), ("max_samples", C.c_uint32), ("batch_samples", C.c_uint32), ("max_above", C.c_uint64)]


class NoiseResult(C.Structure):
    """rpt_noise_result"""
    _fields_ = [("samples_rendered", C.c_uint32), ("converged", C.c_uint32), ("counts", NoiseCounts), ("ms", C.c_double)]


class AdaptiveResult(C.Structure):
    """rpt_adaptive_result"""
    _fields_ = [("passes", C.c_uint32), ("converged", C.c_uint32), ("min_pixel_samples", C.c_uint32), ("max_pixel_samples", C.c_uint32),
                ("pixel_samples", C.c_uint64), ("counts", NoiseCounts), ("ms", C.c_double)]


class GatheredInfo(C.Structure):
    """rpt_gathered_info"""
    _fields_ = [("with_moments", C.c_uint32), ("nonuniform", C.c_uint32), ("samples_min", C.c_uint32), ("samples_max", C.c_uint32), ("bad_trailers", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class GuidesInfo(C.Structure):
    """rpt_guides_info"""
    _fields_ = [("max_interfaces", C.c_uint32), ("rounds", C.c_uint32), ("rays", C.c_uint32 * 9), ("pixels_through_glass", C.c_uint32), ("pixels_exhausted", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


GUIDES_MAX_INTERFACES = 8       # rpt_set_guides_through_glass takes 0 .. 8; the setting ships off (0)
# the recommended budget: the K of the lowest summed rel-L2 over the pixels that look through glass in profiles/r20_glass_guides_quality.txt
# (tools/denoise_probe.py --quality-glass; tests/test_guides_glass.py holds it to that file)
GUIDES_THROUGH_GLASS = 2
GATHER_FORMAT = 0x52504D32     # RPT_GATHER_FORMAT (rpt_debug.h): word 0 of a rank's trailer


def _gathered_info_dict(g):
    return {k: getattr(g, k) for k in ("with_moments", "nonuniform", "samples_min", "samples_max", "bad_trailers")}


def _counts_dict(k):
    return {"pixels": k.pixels, "measured": k.measured, "above": k.above}


def _noise_result_dict(res):
    return {"samples_rendered": res.samples_rendered, "converged": res.converged, "counts": _counts_dict(res.counts), "ms": res.ms}


def _adaptive_result_dict(res):
    return {"passes": res.passes, "converged": res.converged, "min_pixel_samples": res.min_pixel_samples, "max_pixel_samples": res.max_pixel_samples,
            "pixel_samples": res.pixel_samples, "counts": _counts_dict(res.counts), "ms": res.ms}


def denoise_params(**changes):
    """rpt_denoise_params_default, with the named fields replaced: denoise_params(iterations=3, demodulate=0)"""
    p = DenoiseParams()
    lib().rpt_denoise_params_default(C.byref(p))
    for k, v in changes.items():
        if k not in ("iterations", "normal_power_log2", "sigma_color", "sigma_plane", "demodulate"):
            raise TypeError(f"rpt_denoise_params has no field {k}")
        setattr(p, k, v)
    return p


_VAR_FIELDS = ("sigma_variance", "clamp_scale", "clamp_floor", "clamp_radius")
# The firefly clamp ships off.  The lowest summed ratios of profiles/r16_firefly_quality.txt: denoise_var_params(**FIREFLY_CLAMP_VARIANCE) for
# rpt_denoise_variance at 8 spp, temporal_params(**FIREFLY_CLAMP_TEMPORAL) for the eight-view path (tests/test_denoise_firefly.py holds them to the kept grid)
FIREFLY_CLAMP_VARIANCE = {"clamp_scale": 2.0, "clamp_floor": 0.0, "clamp_radius": 1}
FIREFLY_CLAMP_TEMPORAL = {"clamp_scale": 1.0, "clamp_floor": 0.0, "clamp_radius": 3}
# render_adaptive_window: radius 0 .. ADAPTIVE_MAX_RADIUS (RPT_ADAPTIVE_MAX_RADIUS).  ADAPTIVE_WINDOW_RADIUS: the radius with the lowest summed rel-L2 of the grid
# kept in profiles/r17_adaptive_window_quality.txt (tests/test_adaptive_window.py holds it to that file)
ADAPTIVE_MAX_RADIUS = 8
ADAPTIVE_WINDOW_RADIUS = 3


def denoise_var_params(**changes):
    """rpt_denoise_var_params_default, with the named fields replaced; the fields of rpt_denoise_params go into .base:
    denoise_var_params(sigma_variance=4, iterations=5, clamp_scale=2, clamp_radius=2)"""
    p = DenoiseVarParams()
    lib().rpt_denoise_var_params_default(C.byref(p))
    for k, v in changes.items():
        if k in _VAR_FIELDS:
            setattr(p, k, v)
        elif k in ("iterations", "normal_power_log2", "sigma_color", "sigma_plane", "demodulate"):
            setattr(p.base, k, v)
        else:
            raise TypeError(f"rpt_denoise_var_params has no field {k}")
    return p


def temporal_params(**changes):
    """rpt_temporal_params_default, with the named fields replaced; the fields of rpt_denoise_var_params go into .filter and those of rpt_denoise_params
    into .filter.base: temporal_params(max_history=16, sigma_variance=4, iterations=3)"""
    p = TemporalParams()
    lib().rpt_temporal_params_default(C.byref(p))
    for k, v in changes.items():
        if k in ("max_history", "normal_min", "plane_max"):
            setattr(p, k, v)
        elif k in _VAR_FIELDS:
            setattr(p.filter, k, v)
        elif k in ("iterations", "normal_power_log2", "sigma_color", "sigma_plane", "demodulate"):
            setattr(p.filter.base, k, v)
        else:
            raise TypeError(f"rpt_temporal_params has no field {k}")
    return p


def lib_path():
    # RPT_HIP_LIB: developer override used for A/B runs of differently tuned builds
    return os.environ.get("RPT_HIP_LIB") or os.path.join(_ffi.LIB_DIR, "librpt_hip.so")


_SCENE = [C.c_void_p, C.c_size_t] * 5 + [C.c_void_p, C.c_uint32, C.c_uint32] * 2      # rpt_upload_scene after the handle: five buffers with counts, atlas, skybox
_OUT_U32, _OUT_U64, _OUT_SIZE, _OUT_F64, _OUT_PTR = (C.POINTER(t) for t in (C.c_uint32, C.c_uint64, C.c_size_t, C.c_double, C.c_void_p))

# every function of include/rpt/rpt.h and rpt_debug.h, in their order: name -> (return type, [parameter types]); tests/test_contracts.py holds it against the headers.
# (rpt_ctx * and rpt_multi * are c_void_p; so is every buffer a numpy array is handed to through ptr())
PROTOTYPES = {
    "rpt_create": (C.c_int, [C.c_int, _OUT_PTR]),
    "rpt_set_partition": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "rpt_set_samples_in_flight": (C.c_int, [C.c_void_p, C.c_int]),
    "rpt_upload_scene": (C.c_int, [C.c_void_p] + _SCENE),
    "rpt_set_config": (C.c_int, [C.c_void_p, C.POINTER(TracingConfig)]),
    "rpt_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "rpt_render": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_render_async": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_wait": (C.c_int, [C.c_void_p]),
    "rpt_stream": (C.c_int, [C.c_void_p, _OUT_PTR]),
    "rpt_read_accum": (C.c_int, [C.c_void_p, C.c_void_p, _OUT_U32]),
    "rpt_map_accum": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(C.c_float)), _OUT_U32]),
    "rpt_resolve": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "rpt_read_rng": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpt_tile_order": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t, _OUT_SIZE]),
    "rpt_local_pixels": (C.c_int, [C.c_void_p, _OUT_U64]),
    "rpt_local_block_device_ptr": (C.c_int, [C.c_void_p, _OUT_PTR]),
    "rpt_rank_pixels": (C.c_int, [C.c_void_p, C.c_uint32, _OUT_U64]),
    "rpt_untile": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "rpt_comm_unique_id": (C.c_int, [C.c_void_p]),
    "rpt_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32]),
    "rpt_comm_init_local": (C.c_int, [C.c_void_p]),
    "rpt_comm_world": (C.c_int, [C.c_void_p, _OUT_U32, _OUT_U32]),
    "rpt_comm_library": (C.c_char_p, []),
    "rpt_gather_async": (C.c_int, [C.c_void_p]),
    "rpt_gather_wait": (C.c_int, [C.c_void_p]),
    "rpt_read_gathered": (C.c_int, [C.c_void_p, C.c_void_p, _OUT_U32]),
    "rpt_gathered_device_ptr": (C.c_int, [C.c_void_p, _OUT_PTR]),
    "rpt_gather_set_moments": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_gather_moments": (C.c_int, [C.c_void_p, _OUT_U32]),
    "rpt_read_gathered_moments": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpt_gathered_moments_device_ptr": (C.c_int, [C.c_void_p, _OUT_PTR]),
    "rpt_gathered_info_get": (C.c_int, [C.c_void_p, C.POINTER(GatheredInfo)]),
    "rpt_multi_create": (C.c_int, [C.POINTER(C.c_int), C.c_int, C.c_uint32, _OUT_PTR]),
    "rpt_multi_size": (C.c_int, [C.c_void_p]),
    "rpt_multi_ctx": (C.c_void_p, [C.c_void_p, C.c_int]),
    "rpt_multi_upload_scene": (C.c_int, [C.c_void_p] + _SCENE),
    "rpt_multi_set_config": (C.c_int, [C.c_void_p, C.POINTER(TracingConfig)]),
    "rpt_multi_reset": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "rpt_multi_set_shadow_mode": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_multi_render": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_multi_wait": (C.c_int, [C.c_void_p]),
    "rpt_multi_read_accum": (C.c_int, [C.c_void_p, C.c_void_p, _OUT_U32]),
    "rpt_multi_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "rpt_multi_destroy": (None, [C.c_void_p]),
    "rpt_multi_last_error": (C.c_char_p, [C.c_void_p]),
    "rpt_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "rpt_destroy": (None, [C.c_void_p]),
    "rpt_last_error": (C.c_char_p, [C.c_void_p]),
    "rpt_abi_version": (C.c_int, []),
    "rpt_build_fingerprint": (C.c_char_p, []),
    "rpt_device_info": (C.c_int, [C.c_int, _OUT_U32, _OUT_U32]),
    "rpt_shadow_order": (C.c_int, [C.c_void_p, _OUT_U32, _OUT_F64, _OUT_F64, _OUT_U32, _OUT_F64]),
    "rpt_set_shadow_mode": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_shadow_mode": (C.c_int, [C.c_void_p, _OUT_U32]),
    "rpt_set_material_models": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rpt_material_models": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _OUT_SIZE]),
    "rpt_multi_set_material_models": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rpt_set_material_volumes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rpt_material_volumes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _OUT_SIZE]),
    "rpt_multi_set_material_volumes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "rpt_set_punctual_lights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]),
    "rpt_punctual_lights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, _OUT_SIZE, C.c_void_p]),
    "rpt_multi_set_punctual_lights": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float]),
    "rpt_camera_lens_default": (None, [C.c_void_p]),
    "rpt_set_camera_lens": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpt_camera_lens_get": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpt_multi_set_camera_lens": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpt_last_bounce_order": (C.c_int, [C.c_void_p, _OUT_U32, _OUT_U32, _OUT_F64, _OUT_U32, _OUT_F64]),
    "rpt_denoise_params_default": (None, [C.POINTER(DenoiseParams)]),
    "rpt_denoise": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(DenoiseParams), C.c_uint32, C.c_void_p, C.POINTER(DenoiseReport)]),
    "rpt_read_guides": (C.c_int, [C.c_void_p] + [C.c_void_p] * 5),
    "rpt_multi_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseParams), C.c_uint32, C.c_void_p, C.POINTER(DenoiseReport)]),
    "rpt_set_guides_through_glass": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_guides_through_glass": (C.c_int, [C.c_void_p, _OUT_U32]),
    "rpt_guides_info_get": (C.c_int, [C.c_void_p, C.POINTER(GuidesInfo)]),
    "rpt_multi_set_guides_through_glass": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_set_moments": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_moments": (C.c_int, [C.c_void_p, _OUT_U32]),
    "rpt_read_moments": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpt_read_noise": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpt_noise_count": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(NoiseCounts)]),
    "rpt_render_to_noise": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.POINTER(NoiseResult)]),
    "rpt_multi_set_moments": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_multi_read_moments": (C.c_int, [C.c_void_p, C.c_void_p]),
    "rpt_multi_gather_set_moments": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rpt_multi_noise_count": (C.c_int, [C.c_void_p, C.c_float, C.POINTER(NoiseCounts)]),
    "rpt_multi_render_to_noise": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.POINTER(NoiseResult)]),
    "rpt_denoise_var_params_default": (None, [C.POINTER(DenoiseVarParams)]),
    "rpt_denoise_variance": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(DenoiseVarParams), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(DenoiseReport)]),
    "rpt_multi_denoise_variance": (C.c_int, [C.c_void_p, C.POINTER(DenoiseVarParams), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(DenoiseReport)]),
    "rpt_temporal_params_default": (None, [C.POINTER(TemporalParams)]),
    "rpt_denoise_temporal": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(TemporalParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TemporalReport)]),
    "rpt_temporal_reset": (C.c_int, [C.c_void_p]),
    "rpt_multi_denoise_temporal": (C.c_int, [C.c_void_p, C.POINTER(TemporalParams), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(TemporalReport)]),
    "rpt_multi_temporal_reset": (C.c_int, [C.c_void_p]),
    "rpt_render_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rpt_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.POINTER(AdaptiveResult)]),
    "rpt_counts_uniform": (C.c_int, [C.c_void_p, _OUT_U32]),
    "rpt_multi_render_pixels": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "rpt_multi_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.POINTER(AdaptiveResult)]),
    "rpt_render_adaptive_window": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.c_uint32, C.POINTER(AdaptiveResult)]),
    "rpt_multi_render_adaptive_window": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.c_uint32, C.POINTER(AdaptiveResult)]),
    "rpt_adaptive_mask": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.c_uint32, C.c_void_p, C.POINTER(NoiseCounts)]),
    "rpt_multi_adaptive_mask": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.c_uint32, C.c_void_p, C.POINTER(NoiseCounts)]),
    "rpt_bvh_build_gpu": (C.c_int, [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_uint32, C.c_void_p, C.c_size_t, _OUT_SIZE, _OUT_F64]),
    "rpt_light_table_build_gpu": (C.c_int, [C.c_int] + [C.c_void_p, C.c_size_t] * 4 + [_OUT_SIZE, _OUT_U32, _OUT_F64]),
    "rpt_debug_math": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rpt_debug_math_host": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rpt_debug_shadow_order_host": (C.c_int, [C.c_void_p, C.c_size_t] * 5 + [_OUT_U32, _OUT_F64, _OUT_F64, _OUT_U32, C.c_void_p]),
    "rpt_debug_shadow_order_why": (C.c_char_p, [C.c_void_p]),
    "rpt_debug_last_order_host": (C.c_int, [C.c_void_p, C.c_size_t] * 4 + [_OUT_U32, _OUT_F64, _OUT_U32, C.c_void_p]),
    "rpt_debug_math_sweep": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, C.c_float, _OUT_U64, _OUT_U32]),
    "rpt_debug_rcp": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]),
    "rpt_debug_rcp_sweep": (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint64, _OUT_U64, C.c_void_p]),
    "rpt_debug_trace_rays": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 6),
    "rpt_debug_trace_rays_production": (C.c_int, [C.c_void_p, C.c_size_t] + [C.c_void_p] * 5),
    "rpt_debug_walk_production": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t] + [C.c_void_p] * 6),
    "rpt_debug_bsdf": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rpt_debug_sample_image": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rpt_debug_comm_selftest": (C.c_int, [C.c_void_p, C.c_uint32, _OUT_U64]),
    "rpt_debug_denoise_host": (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.POINTER(DenoiseParams), C.c_uint32, C.c_void_p]),
    "rpt_debug_denoise_variance_host": (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.POINTER(DenoiseVarParams), C.c_uint32, C.c_void_p, C.c_void_p]),
    "rpt_debug_denoise_temporal_host": (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 7 + [C.POINTER(TracingConfig), C.POINTER(TracingConfig)] + [C.c_void_p] * 4
                                        + [C.POINTER(TemporalParams), C.c_uint32] + [C.c_void_p] * 4 + [_OUT_U64]),
    "rpt_debug_firefly_host": (C.c_int, [C.c_uint32, C.c_uint32] + [C.c_void_p] * 5 + [C.c_uint32, C.c_float, C.c_float, C.c_uint32, C.c_uint32] + [C.c_void_p] * 3),
    "rpt_debug_glass_step_host": (C.c_int, [C.c_void_p, C.c_size_t] * 3 + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_size_t] + [C.c_void_p] * 13),
    "rpt_debug_noise_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.POINTER(NoiseCounts)]),
    "rpt_debug_adaptive_select_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, _OUT_SIZE]),
    "rpt_debug_adaptive_window_host": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "rpt_debug_adaptive_select_ms": (C.c_int, [C.c_void_p, C.POINTER(NoiseTarget), C.c_uint32, C.c_uint32, C.c_void_p]),
    "rpt_debug_gather_layout": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _OUT_U64, _OUT_U64, C.c_void_p, C.c_void_p]),
    "rpt_debug_gather_host": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32] + [C.c_void_p] * 6 + [C.POINTER(GatheredInfo)]),
    "rpt_debug_short_batch": (C.c_int, [C.c_void_p, C.c_int]),
    "rpt_debug_force_model_kernels": (C.c_int, [C.c_void_p, C.c_int]),
    "rpt_debug_force_volume_kernels": (C.c_int, [C.c_void_p, C.c_int]),
    "rpt_debug_last_shade_variant": (C.c_int, [C.c_void_p, _OUT_U32]),
    "rpt_debug_volume_transmit": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "rpt_debug_lens_rays_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rpt_debug_lens_rays": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "rpt_debug_force_punctual_kernels": (C.c_int, [C.c_void_p, C.c_int]),
    "rpt_debug_punctual_lights_check": (C.c_int, [C.c_void_p, C.c_size_t, C.c_float, C.c_int, C.c_void_p, C.c_size_t]),
    "rpt_debug_punctual_sample_host": (C.c_int, [C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5),
    "rpt_debug_punctual_sample": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_void_p, C.c_void_p, C.c_size_t] + [C.c_void_p] * 5),
}
EXPORTS = sorted(PROTOTYPES)


def lib():
    """librpt_hip.so with the prototypes of PROTOTYPES.  The in-tree library must have every one of them; the build RPT_HIP_LIB names may be an older one
    (an A/B run against a library without shadow modes or moments): what it lacks is left out, and calling it raises AttributeError."""
    global _lib
    if _lib is None:
        path = lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} is missing: run `make hip` (or __graft_entry__.build()); there is no CPU fallback")
        _lib = _ffi.bind(C.CDLL(path), PROTOTYPES, allow_missing=bool(os.environ.get("RPT_HIP_LIB")))
    return _lib


class RptError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"librpt_hip error {code}: {message}")
        self.code = code


_COUNTERS = ("samples", "extension_rays", "shadow_rays", "shadow_rays_elided", "sky_evals", "light_index_clamped", "iterations")


class _Handle:
    """What Renderer (an rpt_ctx, prefix rpt_) and MultiRenderer (an rpt_multi, prefix rpt_multi_) share: the handle, its error text, and the entry
    points whose C signatures are equal after the handle.  `_call("render", n)` is rpt_render(h, n) or rpt_multi_render(h, n), checked."""
    _prefix = None

    def _fn(self, name):
        return getattr(lib(), self._prefix + name)

    def _open(self, create, *args):
        self._h = C.c_void_p()
        rc = create(*args, C.byref(self._h))
        if rc != 0:
            raise RptError(rc, self._fn("last_error")(None).decode())

    def _check(self, rc):
        if rc != 0:
            raise RptError(rc, self._fn("last_error")(self._h).decode())

    def _call(self, name, *args):
        self._check(self._fn(name)(self._h, *args))

    def close(self):
        if getattr(self, "_h", None):
            if not getattr(self, "_borrowed", False):
                self._fn("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _image(self, *channels, dtype=np.float32):
        """zeros of (H, W) + channels for a read-out of the configured size"""
        return np.zeros((self.config.height, self.config.width) + channels, dtype)

    # -- rpt_upload_scene <-> World::into_gpu (reference: src/asset.rs:226-235)
    def upload_scene(self, world, skybox_f32=None):
        atlas = getattr(world, "atlas", None)
        aw = ah = sw = sh = 0
        if atlas is not None:
            atlas = np.ascontiguousarray(atlas, np.uint8)
            ah, aw = atlas.shape[:2]
        if skybox_f32 is not None:
            skybox_f32 = np.ascontiguousarray(skybox_f32, np.float32)
            sh, sw = skybox_f32.shape[:2]
        self._call("upload_scene", ptr(world.per_vertex), len(world.per_vertex), ptr(world.indices), len(world.indices),
                   ptr(world.nodes), len(world.nodes), ptr(world.materials), len(world.materials),
                   ptr(world.light_pick), len(world.light_pick), ptr(atlas), aw, ah, ptr(skybox_f32), sw, sh)

    # -- rpt_set_config <-> config_buffer write (reference: src/trace.rs:168,219)
    def set_config(self, config):
        self._call("set_config", C.byref(config))
        self.config = config.copy()

    # -- rpt_reset <-> rng/output buffer creation + flush (reference: src/trace.rs:164-170,219-221)
    def reset(self, rng_seed, accum_init=None, samples_init=0):
        rng_seed = np.ascontiguousarray(rng_seed, RNG_DTYPE)
        if accum_init is not None:
            accum_init = np.ascontiguousarray(accum_init, np.float32)
        self._call("reset", ptr(rng_seed), ptr(accum_init), samples_init)

    # -- rpt_render <-> the enqueue/poll loop (reference: src/trace.rs:182-194)
    def render(self, n_samples):
        self._call("render", n_samples)

    def wait(self):
        self._call("wait")

    # -- rpt_read_accum <-> output_buffer.read_blocking (reference: src/trace.rs:198)
    def read_accum(self, out=None):
        if out is None:
            out = self._image(4)
        assert out.dtype == np.float32 and out.size == self.config.height * self.config.width * 4 and out.flags["C_CONTIGUOUS"]
        samples = C.c_uint32()
        self._call("read_accum", ptr(out), C.byref(samples))
        return out, samples.value

    def _denoise(self, source, params, tonemap_op, with_report):
        """source: what rpt_denoise takes between the handle and params, as a tuple (rpt_multi_denoise: nothing)"""
        out, rep = self._image(3), DenoiseReport()
        self._call("denoise", *source, None if params is None else C.byref(params), tonemap_op, ptr(out), C.byref(rep))
        return (out, _report_dict(rep)) if with_report else out

    def _denoise_variance(self, source, params, tonemap_op, with_report):
        """source: what rpt_denoise_variance takes between the handle and params, as a tuple (rpt_multi_denoise_variance: nothing)"""
        out, var, rep = self._image(3), self._image(), DenoiseReport()
        self._call("denoise_variance", *source, None if params is None else C.byref(params), tonemap_op, ptr(out), ptr(var), C.byref(rep))
        return (out, var, _report_dict(rep)) if with_report else (out, var)

    def _denoise_temporal(self, source, params, tonemap_op, with_report):
        """source: what rpt_denoise_temporal takes between the handle and params, as a tuple (rpt_multi_denoise_temporal: nothing)"""
        out, var, hist, rep = self._image(3), self._image(), self._image(), TemporalReport()
        self._call("denoise_temporal", *source, None if params is None else C.byref(params), tonemap_op, ptr(out), ptr(var), ptr(hist), C.byref(rep))
        report = dict(_report_dict(rep.base), pixels_with_history=rep.pixels_with_history, history_state=rep.history_state)
        return (out, var, hist, report) if with_report else (out, var, hist)

    def temporal_reset(self):
        """rpt_temporal_reset (rpt_multi_: on rank 0, where it lives): forget and free the history of denoise_temporal"""
        self._call("temporal_reset")

    def set_shadow_mode(self, mode):
        """rpt_set_shadow_mode (rpt_multi_: on every rank): SHADOW_EXACT (default: the reference's any-hit walk, bit for bit) or SHADOW_SEGMENT (boxes that begin
        behind the ray's max_t are not entered: faster, an occlusion can in principle be lost); holds for the batches enqueued afterwards."""
        self._call("set_shadow_mode", mode)

    def set_material_models(self, records=None):
        """rpt_set_material_models (rpt_multi_: on every rank): one record per material of the uploaded scene (material_models(...), or an array of
        MATERIAL_MODEL_DTYPE) — MODEL_PBR, MODEL_LAMBERTIAN or MODEL_GLASS with its ior — in place of the BSDF the reference constructs at lib.rs:144;
        None: every material PBR again.  Between batches; accumulator, rng, moments and statistics stay; upload_scene clears the records."""
        if records is None:
            self._call("set_material_models", None, 0)
            return
        records = np.ascontiguousarray(records, MATERIAL_MODEL_DTYPE)
        self._call("set_material_models", ptr(records), len(records))

    def set_material_volumes(self, records=None):
        """rpt_set_material_volumes (rpt_multi_: on every rank): one absorption record per material of the uploaded scene (material_volumes(...), or an array
        of MATERIAL_VOLUME_DTYPE): a path segment that reaches a MODEL_GLASS surface from its inside is attenuated by exp(-sigma * length) per channel.
        None: no records.  Between batches; accumulator, rng, moments, statistics and guides stay; upload_scene clears the records."""
        if records is None:
            self._call("set_material_volumes", None, 0)
            return
        records = np.ascontiguousarray(records, MATERIAL_VOLUME_DTYPE)
        self._call("set_material_volumes", ptr(records), len(records))

    def set_punctual_lights(self, lights=None, pick_share=0.5):
        """rpt_set_punctual_lights (rpt_multi_: on every rank): point, spot and directional lights (punctual_lights(point_light(..), spot_light(..), ..), or an
        array of PUNCTUAL_LIGHT_DTYPE) sampled by next-event estimation — NEE modes 1 and 2 only; pick_share: the share of light picks they take from the
        scene's emissive triangles, in (0, 1) (ignored, 1, where the scene has none).  None or empty: no lights.  Between batches; the caller resets the
        accumulator; upload_scene clears the lights."""
        if lights is None or len(lights) == 0:
            self._call("set_punctual_lights", None, 0, float(pick_share))
            return
        lights = np.ascontiguousarray(lights, PUNCTUAL_LIGHT_DTYPE).reshape(-1)
        self._call("set_punctual_lights", ptr(lights), len(lights), float(pick_share))

    def set_camera_lens(self, lens=None, **fields):
        """rpt_set_camera_lens (rpt_multi_: on every rank): a CameraLens, or its fields by name (tan_half_fov — see hip.tan_half_fov(degrees) —, aperture_radius,
        focus_distance); None and no field: the reference's pinhole again.  Holds from the next render call; the caller resets the accumulator."""
        if lens is None and fields:
            lens = camera_lens(**fields)
        self._call("set_camera_lens", None if lens is None else C.byref(lens))

    def set_guides_through_glass(self, max_interfaces):
        """rpt_set_guides_through_glass (rpt_multi_: on every rank): 0 (default) first-hit guides; 1 .. GUIDES_MAX_INTERFACES: the denoiser's guides follow
        MODEL_GLASS materials through that many interfaces to the surface seen through them (albedo = the tints crossed x that surface's, depth = the summed
        path, position on the pixel's own ray).  The guides are rebuilt at their next use."""
        self._call("set_guides_through_glass", max_interfaces)

    # -- per-pixel sample moments and the noise estimate (no reference equivalent; include/rpt/rpt.h "per-pixel sample moments")
    def set_moments(self, on=True):
        """rpt_set_moments (rpt_multi_: on every rank): keep (sum Y, sum Y^2, n, max Y) of every pixel's samples beside the accumulator; turning it on zeroes the
        record.  The image does not depend on it.  A renderer with one sample of a pixel in flight (set_samples_in_flight(1)) refuses to render while it is on."""
        self._call("set_moments", 1 if on else 0)

    def read_moments(self):
        """rpt_read_moments: (H, W, 4) float32 — sum of luminance, sum of its square, samples since the record was zeroed, brightest sample; other ranks' pixels 0
        (rpt_multi_: the whole image, the ranks' records merged on the host)"""
        out = self._image(4)
        self._call("read_moments", ptr(out))
        return out

    def noise_count(self, threshold):
        """rpt_noise_count (rpt_multi_: summed over the ranks): {"pixels": owned, "measured": with two samples or more, "above": measured with not (rel <= threshold)}"""
        k = NoiseCounts()
        self._call("noise_count", threshold, C.byref(k))
        return _counts_dict(k)

    def render_to_noise(self, threshold, max_above=0, batch_samples=32, min_samples=32, max_samples=1024):
        """rpt_render_to_noise: batches of batch_samples until every pixel is measured and at most max_above are above threshold (counted from min_samples on),
        or max_samples are rendered: {"samples_rendered", "converged", "counts", "ms"}.  Turns moments on and leaves them on.
        (rpt_multi_: over every GPU, each batch gathered as render() gathers it)"""
        t, res = NoiseTarget(threshold, min_samples, max_samples, batch_samples, max_above), NoiseResult()
        self._call("render_to_noise", C.byref(t), C.byref(res))
        return _noise_result_dict(res)

    # -- chosen pixels (include/rpt/rpt.h "chosen pixels")
    def render_pixels(self, mask, n_samples):
        """rpt_render_pixels (rpt_multi_: every rank among its own pixels, then the gather): n_samples more samples for the pixels whose entry of `mask`
        (H, W), any dtype, is non-zero.  Returns once enqueued when the batch's length is known, as render_async."""
        mask = np.ascontiguousarray(np.asarray(mask) != 0, np.uint8)
        assert mask.size == self.config.height * self.config.width
        self._call("render_pixels", ptr(mask), n_samples)

    def render_adaptive(self, threshold, max_above=0, batch_samples=8, min_samples=8, max_samples=256):
        """rpt_render_adaptive: min_samples for every pixel, then passes of batch_samples for the pixels whose noise is not yet at or below threshold and
        that stay within max_samples, until at most max_above are above or nothing is selected: {"passes", "converged", "min_pixel_samples",
        "max_pixel_samples", "pixel_samples", "counts", "ms"}.  Turns moments on and leaves them on."""
        t, res = NoiseTarget(threshold, min_samples, max_samples, batch_samples, max_above), AdaptiveResult()
        self._call("render_adaptive", C.byref(t), C.byref(res))
        return _adaptive_result_dict(res)

    def render_adaptive_window(self, radius, threshold, max_above=0, batch_samples=8, min_samples=8, max_samples=256):
        """rpt_render_adaptive_window: render_adaptive, but a pixel is selected while ANY pixel within `radius` (0 .. ADAPTIVE_MAX_RADIUS; clipped to the
        pixel's 64 x 64 tile) is above the threshold, so pixels whose few samples happen to agree are not abandoned beside noisy ones.  radius 0 is
        render_adaptive.  The same result dictionary; counts are still about each pixel's own noise."""
        t, res = NoiseTarget(threshold, min_samples, max_samples, batch_samples, max_above), AdaptiveResult()
        self._call("render_adaptive_window", C.byref(t), radius, C.byref(res))
        return _adaptive_result_dict(res)

    def adaptive_mask(self, radius, threshold, max_above=0, batch_samples=8, min_samples=8, max_samples=256):
        """rpt_adaptive_mask (rpt_multi_: the ranks' masks merged, their counts summed): (the pixels the next pass of render_adaptive_window would render as
        (H, W) uint8, the counts of noise_count).  Renders nothing; render_pixels(mask, batch_samples) is that pass.  Moments must be on."""
        t, k, mask = NoiseTarget(threshold, min_samples, max_samples, batch_samples, max_above), NoiseCounts(), self._image(dtype=np.uint8)
        self._call("adaptive_mask", C.byref(t), radius, ptr(mask), C.byref(k))
        return mask, _counts_dict(k)

    def _get_stats(self):
        s = Stats()
        self._call("get_stats", C.byref(s))
        return s


class Renderer(_Handle):
    """One rpt_ctx on one GPU (one process per GPU in multi-GPU runs)."""
    _prefix = "rpt_"

    def __init__(self, device_id=0, rank=0, world_size=1):
        self._open(lib().rpt_create, device_id)
        self.rank, self.world_size = rank, world_size
        if world_size != 1:
            self._check(lib().rpt_set_partition(self._h, rank, world_size))
        self.config = None

    @classmethod
    def borrowed(cls, handle, config=None, rank=0, world_size=1):
        """A view of an rpt_ctx somebody else owns (rpt_multi_ctx): every method works, close() / garbage collection leave the context alone."""
        self = cls.__new__(cls)
        self._h, self._borrowed = handle, True
        self.rank, self.world_size, self.config = rank, world_size, config
        return self

    def set_partition(self, rank, world_size):
        """rpt_set_partition: this context renders the tiles of `rank` of `world_size` (state is re-allocated at the next reset)."""
        self._check(lib().rpt_set_partition(self._h, rank, world_size))
        self.rank, self.world_size = rank, world_size

    def set_samples_in_flight(self, samples):
        """0 = automatic. Never changes the result (tests/test_gpu_parity.py::test_samples_in_flight_invisible)."""
        self._check(lib().rpt_set_samples_in_flight(self._h, samples))

    def reset(self, rng_seed, accum_init=None, samples_init=0):
        """(the sizes are checked here; a MultiRenderer leaves that to rpt_multi_reset)"""
        rng_seed = np.ascontiguousarray(rng_seed, RNG_DTYPE)
        assert rng_seed.size == self.config.width * self.config.height
        assert accum_init is None or np.size(accum_init) == rng_seed.size * 4
        super().reset(rng_seed, accum_init, samples_init)

    def render_async(self, n_samples):
        """rpt_render_async: returns once the batch is enqueued when its iteration count is known (n_samples <= slots per
        pixel), else behaves like render()."""
        self._check(lib().rpt_render_async(self._h, n_samples))

    def stream_ptr(self):
        """The hipStream_t the library enqueues on (wrap with torch.cuda.ExternalStream to order work after a batch)."""
        p = C.c_void_p()
        self._check(lib().rpt_stream(self._h, C.byref(p)))
        return p.value

    def map_accum(self):
        """rpt_map_accum: the library's own pinned read-back buffer as an (H, W, 4) array — no copy; valid until the
        next read_accum / map_accum / set_config on this renderer."""
        p = C.POINTER(C.c_float)()
        samples = C.c_uint32()
        self._check(lib().rpt_map_accum(self._h, C.byref(p), C.byref(samples)))
        return np.ctypeslib.as_array(p, shape=(self.config.height, self.config.width, 4)), samples.value

    def resolve(self, tonemap_op=0):
        """mean radiance (+ display tonemap 0..6, reference: src/resources/render.wgsl:131-153) as (H, W, 3) float32."""
        out = self._image(3)
        self._check(lib().rpt_resolve(self._h, tonemap_op, ptr(out)))
        return out

    # -- rpt_denoise <-> the denoise step of the read-back (reference: src/trace.rs:205-213)
    def denoise(self, source=DENOISE_ACCUM, params=None, tonemap_op=0, with_report=False):
        """rpt_denoise: the mean image filtered by the guided a-trous filter, then tonemapped, as (H, W, 3) float32 (params None: the defaults;
        with_report: also {"device_ms", "guides_ms", "guides_rebuilt"})."""
        return self._denoise((source,), params, tonemap_op, with_report)

    def denoise_variance(self, source=DENOISE_ACCUM, moments=None, params=None, tonemap_op=0, with_report=False):
        """rpt_denoise_variance: denoise() with the luminance term that the per-pixel variance of the mean drives (params: denoise_var_params(), None: the
        defaults).  moments None: the renderer's own record (set_moments first) with DENOISE_ACCUM, the gathered record (gather_set_moments first) with
        DENOISE_GATHERED; else an (H, W, 4) image as read_moments() returns.
        Returns (rgb (H, W, 3), variance (H, W): the filtered variance of the mean luminance, inf = unknown)[, report]."""
        if moments is not None:
            moments = np.ascontiguousarray(moments, np.float32)
            assert moments.shape == (self.config.height, self.config.width, 4)
        return self._denoise_variance((source, ptr(moments)), params, tonemap_op, with_report)

    def denoise_temporal(self, source=DENOISE_ACCUM, moments=None, params=None, tonemap_op=0, with_report=False):
        """rpt_denoise_temporal: denoise_variance() with the previous view's history reprojected and blended in front of the passes (params:
        temporal_params(), None: the defaults; moments as denoise_variance).  Returns (rgb (H, W, 3), variance (H, W), history (H, W): the blended sample
        count T of every pixel)[, report: that of denoise() and {"pixels_with_history", "history_state": HISTORY_NONE / USED / DROPPED}]."""
        if moments is not None:
            moments = np.ascontiguousarray(moments, np.float32)
            assert moments.shape == (self.config.height, self.config.width, 4)
        return self._denoise_temporal((source, ptr(moments)), params, tonemap_op, with_report)

    def guides(self):
        """rpt_read_guides: the guide buffers of the current scene and camera (first-hit guides; after set_guides_through_glass(K > 0), the surface seen through glass):
        {"albedo", "normal", "position": (H, W, 3) float32, "depth": (H, W) float32, "kind": (H, W) uint32 (GUIDE_MISS / SURFACE / EMITTER)}"""
        g = {"albedo": self._image(3), "normal": self._image(3), "depth": self._image(), "position": self._image(3), "kind": self._image(dtype=np.uint32)}
        self._check(lib().rpt_read_guides(self._h, ptr(g["albedo"]), ptr(g["normal"]), ptr(g["depth"]), ptr(g["position"]), ptr(g["kind"])))
        return g

    def guides_through_glass(self):
        """rpt_guides_through_glass: the budget of interfaces the guides follow glass through (0: first-hit guides, the default)"""
        k = C.c_uint32()
        self._check(lib().rpt_guides_through_glass(self._h, C.byref(k)))
        return k.value

    def guides_info(self):
        """rpt_guides_info_get: {"max_interfaces": the setting, "rounds": walks of the last guide build (0: none yet), "rays": rays walked per round (9 entries),
        "pixels_through_glass": pixels whose chain crossed an interface, "pixels_exhausted": pixels whose chain ended on a glass surface}"""
        g = GuidesInfo()
        self._check(lib().rpt_guides_info_get(self._h, C.byref(g)))
        return {"max_interfaces": g.max_interfaces, "rounds": g.rounds, "rays": list(g.rays), "pixels_through_glass": g.pixels_through_glass,
                "pixels_exhausted": g.pixels_exhausted}

    def moments_on(self):
        on = C.c_uint32()
        self._check(lib().rpt_moments(self._h, C.byref(on)))
        return bool(on.value)

    def counts_uniform(self):
        """rpt_counts_uniform: False once a masked or adaptive pass has rendered for fewer than all owned pixels (resolve and denoise then divide every pixel
        by its own count), True again after reset"""
        u = C.c_uint32()
        self._check(lib().rpt_counts_uniform(self._h, C.byref(u)))
        return bool(u.value)

    def read_noise(self):
        """rpt_read_noise: (H, W) float32, the standard error of every pixel's mean luminance relative to that mean (inf below two samples); other ranks' pixels 0"""
        out = self._image()
        self._check(lib().rpt_read_noise(self._h, ptr(out)))
        return out

    def read_rng(self):
        out = np.zeros(self.config.height * self.config.width, RNG_DTYPE)
        self._check(lib().rpt_read_rng(self._h, ptr(out)))
        return out

    def stats(self):
        s = self._get_stats()
        d = {k: getattr(s, k) for k in _COUNTERS + ("render_ms",)}
        d["shadow_rays_traced"] = d["shadow_rays"] - d["shadow_rays_elided"]       # walked on the device; shadow_rays counts as the reference does
        d["kernel_ms"] = {n: s.kernel_ms[i] for i, n in enumerate(_ffi.STAGE_NAMES)}
        d["kernel_launches"] = {n: s.kernel_launches[i] for i, n in enumerate(_ffi.STAGE_NAMES)}
        return d

    # -- multi-GPU gather support
    def local_pixels(self):
        n = C.c_uint64()
        self._check(lib().rpt_local_pixels(self._h, C.byref(n)))
        return n.value

    def rank_pixels(self, rank):
        n = C.c_uint64()
        self._check(lib().rpt_rank_pixels(self._h, rank, C.byref(n)))
        return n.value

    def local_block_device_ptr(self):
        p = C.c_void_p()
        self._check(lib().rpt_local_block_device_ptr(self._h, C.byref(p)))
        return p.value

    def untile(self, dev_blocks_ptr, dev_out_ptr, block_stride_pixels=0):
        self._check(lib().rpt_untile(self._h, dev_blocks_ptr, block_stride_pixels, dev_out_ptr))

    # -- the gather inside the library (RCCL): rpt_comm_init / rpt_gather_async / rpt_read_gathered
    def comm_init(self, unique_id, rank, world_size):
        """ncclCommInitRank on this renderer's device + rpt_set_partition(rank, world_size); unique_id = the 128 bytes
        rank 0 got from comm_unique_id(), handed to every rank by any means."""
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        self._check(lib().rpt_comm_init(self._h, buf, rank, world_size))
        self.rank, self.world_size = rank, world_size

    def comm_init_local(self):
        """rpt_comm_init_local: a one-rank communicator without RCCL (overlapped read-back on one GPU)."""
        self._check(lib().rpt_comm_init_local(self._h))

    def shadow_order(self):
        """rpt_shadow_order: {"fixed": bool, "visits_near", "visits_fixed", "probe_rays", "why": the probe's reason} — which (bit-exact) order the shadow walks of the scene use."""
        f, n = C.c_uint32(), C.c_uint32()
        vn, vf, ms = C.c_double(), C.c_double(), C.c_double()
        self._check(lib().rpt_shadow_order(self._h, C.byref(f), C.byref(vn), C.byref(vf), C.byref(n), C.byref(ms)))
        return {"fixed": bool(f.value), "visits_near": vn.value, "visits_fixed": vf.value, "probe_rays": n.value, "probe_ms": ms.value,
                "why": lib().rpt_debug_shadow_order_why(self._h).decode()}

    def material_models(self):
        """rpt_material_models: the records as set, an array of MATERIAL_MODEL_DTYPE (empty: none set)"""
        n = C.c_size_t()
        self._check(lib().rpt_material_models(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, MATERIAL_MODEL_DTYPE)
        self._check(lib().rpt_material_models(self._h, ptr(out), len(out), C.byref(n)))
        return out

    def material_volumes(self):
        """rpt_material_volumes: the records as set, an array of MATERIAL_VOLUME_DTYPE (empty: none set)"""
        n = C.c_size_t()
        self._check(lib().rpt_material_volumes(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, MATERIAL_VOLUME_DTYPE)
        self._check(lib().rpt_material_volumes(self._h, ptr(out), len(out), C.byref(n)))
        return out

    def punctual_lights(self):
        """rpt_punctual_lights: (the records as set, an array of PUNCTUAL_LIGHT_DTYPE — empty: none —, the effective share of the first light draw)"""
        n, q = C.c_size_t(), C.c_float()
        self._check(lib().rpt_punctual_lights(self._h, None, 0, C.byref(n), C.byref(q)))
        out = np.zeros(n.value, PUNCTUAL_LIGHT_DTYPE)
        self._check(lib().rpt_punctual_lights(self._h, ptr(out), len(out), C.byref(n), C.byref(q)))
        return out, q.value

    def debug_force_punctual_kernels(self, on=True):
        """rpt_debug_force_punctual_kernels (test hook): the punctual variant of the shade stage under NEE whatever the lights say"""
        self._check(lib().rpt_debug_force_punctual_kernels(self._h, 1 if on else 0))

    def debug_punctual_sample(self, lights, q, hits, l1):
        """rpt_debug_punctual_sample on the device (test hook): punctual_sample of csrc/k_punctual.h -> (j, L, max_t, E, pick_pdf)"""
        return _punctual_sample(self._h, lights, q, hits, l1)

    def camera_lens(self):
        """rpt_camera_lens_get: the lens as set (a CameraLens)"""
        out = CameraLens()
        self._check(lib().rpt_camera_lens_get(self._h, C.byref(out)))
        return out

    def debug_lens_rays(self, pixels_xy, keys):
        """rpt_debug_lens_rays (test hook): the context's camera rays for (x | y << 16, key) pairs through a device kernel: (origins, dirs), (n, 3) float32 each"""
        pixels_xy, keys = np.ascontiguousarray(pixels_xy, np.uint32), np.ascontiguousarray(keys, np.uint32)
        o, d = np.zeros((len(keys), 3), np.float32), np.zeros((len(keys), 3), np.float32)
        self._check(lib().rpt_debug_lens_rays(self._h, ptr(pixels_xy), ptr(keys), len(keys), ptr(o), ptr(d)))
        return o, d

    def debug_force_model_kernels(self, on=True):
        """rpt_debug_force_model_kernels (test hook): the models variant of the shade stage whatever the records say"""
        self._check(lib().rpt_debug_force_model_kernels(self._h, 1 if on else 0))

    def debug_force_volume_kernels(self, on=True):
        """rpt_debug_force_volume_kernels (test hook): the volumes variant of the shade stage whatever the records say"""
        self._check(lib().rpt_debug_force_volume_kernels(self._h, 1 if on else 0))

    def debug_last_shade_variant(self):
        """rpt_debug_last_shade_variant (test hook): 0 k_shade, 1 k_shade_models, 2 k_shade_volumes, 3 k_shade_punctual — the context's last shade launch"""
        v = C.c_uint32()
        self._check(lib().rpt_debug_last_shade_variant(self._h, C.byref(v)))
        return v.value

    def debug_volume_transmit(self, throughput, sigma, t):
        """rpt_debug_volume_transmit on the device (test hook): vol_transmit of csrc/k_volume.h, (n, 3), (n, 3), (n,) -> (n, 3) float32"""
        return _volume_transmit(self._h, 1, throughput, sigma, t)

    def shadow_mode(self):
        m = C.c_uint32()
        self._check(lib().rpt_shadow_mode(self._h, C.byref(m)))
        return m.value

    LAST_BOUNCE_MODES = ("whole walk", "hit or miss, near child first", "hit or miss, more opaque child first", "hit or miss, smaller subtree first",
                         "hit or miss, more opaque per node first")

    def last_bounce_order(self):
        """rpt_last_bounce_order: how the last extension rays of a batch without NEE are walked on the uploaded scene (every mode gives the same image)."""
        m, ne, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        v = (C.c_double * 4)()
        ms = C.c_double()
        self._check(lib().rpt_last_bounce_order(self._h, C.byref(m), C.byref(ne), v, C.byref(n), C.byref(ms)))
        return {"mode": m.value, "mode_is": self.LAST_BOUNCE_MODES[m.value], "emissive_triangles": ne.value, "probe_rays": n.value, "probe_ms": ms.value,
                "probe_node_visits": {"near child first": v[0], "more opaque first": v[1], "smaller subtree first": v[2], "more opaque per node first": v[3]}}

    def comm_world(self):
        r, w = C.c_uint32(), C.c_uint32()
        self._check(lib().rpt_comm_world(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def comm_selftest(self, n_floats=1 << 20):
        """rpt_debug_comm_selftest: words that differ after a grouped ncclSend / ncclRecv ring (one rank: to and from itself)."""
        bad = C.c_uint64()
        self._check(lib().rpt_debug_comm_selftest(self._h, n_floats, C.byref(bad)))
        return bad.value

    def gather_async(self):
        self._check(lib().rpt_gather_async(self._h))

    def gather_wait(self):
        self._check(lib().rpt_gather_wait(self._h))

    def read_gathered(self, out=None):
        if out is None:
            out = self._image(4)
        samples = C.c_uint32()
        self._check(lib().rpt_read_gathered(self._h, ptr(out), C.byref(samples)))
        return out, samples.value

    # -- the moments record and the counts flag inside the gather (include/rpt/rpt.h "inside the gather")
    def gather_set_moments(self, on=True):
        """rpt_gather_set_moments: the gather also carries this rank's moments record and its count state to rank 0 (turns moments on and leaves them on).
        Collective: every rank of the communicator holds the same value at every gather.  No gathered image exists until the next gather."""
        self._check(lib().rpt_gather_set_moments(self._h, 1 if on else 0))

    def gather_moments(self):
        on = C.c_uint32()
        self._check(lib().rpt_gather_moments(self._h, C.byref(on)))
        return bool(on.value)

    def read_gathered_moments(self):
        """rpt_read_gathered_moments (rank 0): (H, W, 4) float32, the whole image's records as the last gather carried them"""
        out = self._image(4)
        self._check(lib().rpt_read_gathered_moments(self._h, ptr(out)))
        return out

    def gathered_moments_device_ptr(self):
        p = C.c_void_p()
        self._check(lib().rpt_gathered_moments_device_ptr(self._h, C.byref(p)))
        return p.value

    def gathered_info(self):
        """rpt_gathered_info_get (rank 0, waits for the last gather): {"with_moments", "nonuniform", "samples_min", "samples_max", "bad_trailers"}"""
        g = GatheredInfo()
        self._check(lib().rpt_gathered_info_get(self._h, C.byref(g)))
        return _gathered_info_dict(g)

    # -- test hooks (include/rpt/rpt_debug.h)
    def debug_short_batch(self, on=True):
        """rpt_debug_short_batch: asynchronous batches enqueue one iteration too few (the completion checks must notice)."""
        self._check(lib().rpt_debug_short_batch(self._h, 1 if on else 0))

    def debug_math(self, op, x, y=None):
        """rpt_debug_math: one function of csrc/rpt_math.h on the device, elementwise.  op: 0 sin, 1 cos, 2 acos, 3 exp, 4 pow(x, y), 5 asin,
        6 atan2(y=x, x=y), 7 sqrt, 8 IEEE x / y, 9 slab_quotient(x, 0, y), 10 exp_sky, 11 unorm8, 12 fminr(x, y), 13 fmaxr(x, y), 14 floorr, 15 ceilr,
        16 f2u32_sat(x) as the word's bits, 17 atanr, 18 powi5, 19 absr; 20 + 2 k / 21 + 2 k the low / high word of the double that sin_poly, cos_poly,
        exp_core, log_core, asin_poly, atan01 (k = 0 .. 5) return; any other op is refused.  debug_math_host takes the same numbers."""
        x = np.ascontiguousarray(x, np.float32)
        y = x if y is None else np.ascontiguousarray(y, np.float32)
        out = np.empty_like(x)
        self._check(lib().rpt_debug_math(self._h, op, ptr(x), ptr(y), ptr(out), x.size))
        return out

    def debug_math_sweep(self, op, lo_bits, count, y=1.0):
        """rpt_debug_math_sweep: (mismatches, first bad bit pattern) of a cheap exact operation vs its IEEE form."""
        bad, first = C.c_uint64(), C.c_uint32()
        self._check(lib().rpt_debug_math_sweep(self._h, op, lo_bits, count, y, C.byref(bad), C.byref(first)))
        return bad.value, first.value

    def debug_rcp(self, x, window=False):
        """rpt_debug_rcp: rptm::rcp_rn (window: rcp_rn_window) of csrc/rpt_rcp.h on the device, elementwise."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty_like(x)
        self._check(lib().rpt_debug_rcp(self._h, 1 if window else 0, ptr(x), ptr(out), x.size))
        return out

    def debug_rcp_sweep(self, lo_bits, count, window=False):
        """rpt_debug_rcp_sweep: (differences, up to 64 of the differing bit patterns) of rcp_rn (window: rcp_rn_window) vs the device's own 1.0f / x."""
        bad, where = C.c_uint64(), np.zeros(64, np.uint32)
        self._check(lib().rpt_debug_rcp_sweep(self._h, 1 if window else 0, lo_bits, count, C.byref(bad), ptr(where)))
        return bad.value, where[: min(bad.value, 64)]

    def debug_bsdf(self, kind, items):
        """Lambertian / Glass of kernels/src/bsdf.rs:46-176 on the device (rpt_debug_bsdf): (n, 16) in -> (n, 8) out."""
        items = np.ascontiguousarray(items, np.float32).reshape(-1, 16)
        out = np.zeros((len(items), 8), np.float32)
        self._check(lib().rpt_debug_bsdf(self._h, kind, len(items), ptr(items), ptr(out)))
        return out

    def debug_sample_image(self, image, coords_uv):
        """rpt_debug_sample_image: the kernels' sample_by_lod on an image of its own, (h, w, 4) uint8 (an atlas) or float32 (a skybox); coords (n, 2) -> (n, 4)."""
        image = np.ascontiguousarray(image)
        assert image.ndim == 3 and image.shape[2] == 4 and image.dtype in (np.uint8, np.float32)
        coords = np.ascontiguousarray(coords_uv, np.float32).reshape(-1, 2)
        out = np.zeros((len(coords), 4), np.float32)
        self._check(lib().rpt_debug_sample_image(self._h, int(image.dtype == np.uint8), ptr(image), image.shape[1], image.shape[0], len(coords), ptr(coords), ptr(out)))
        return out

    def debug_trace_rays(self, any_hit, origins, dirs, max_t=None):
        """any_hit: 0 / False nearest, 1 / True the reference's any-hit walk, 2 the segment-bounded any-hit walk (rpt_set_shadow_mode)"""
        origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(origins)
        max_t = np.zeros(n, np.float32) if max_t is None else np.ascontiguousarray(max_t, np.float32)
        t = np.zeros(n, np.float32)
        tri = np.zeros(n, np.uint32)
        flags = np.zeros(n, np.uint32)
        self._check(lib().rpt_debug_trace_rays(self._h, 2 if any_hit == 2 else int(bool(any_hit)), n, ptr(origins), ptr(dirs), ptr(max_t),
                                               ptr(t), ptr(tri), ptr(flags)))
        return t, tri, flags

    def debug_trace_rays_production(self, origins, dirs):
        """rpt_debug_trace_rays_production: nearest hits through the traversal stage rpt_render itself launches for this scene / state."""
        origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(origins)
        t = np.zeros(n, np.float32)
        tri = np.zeros(n, np.uint32)
        flags = np.zeros(n, np.uint32)
        self._check(lib().rpt_debug_trace_rays_production(self._h, n, ptr(origins), ptr(dirs), ptr(t), ptr(tri), ptr(flags)))
        return t, tri, flags

    def debug_walk_production(self, kind, origins, dirs, max_t=None):
        """rpt_debug_walk_production: chosen rays through the launch functions of rpt_render — kind WALK_NEAREST_PLAIN / _FIRST (every origin the configuration's
        cam_position) / _LAST, or WALK_SHADOW (max_t per ray; flags bit 0 = occluded, t and triangle stay zero).  Call reset() before rendering again."""
        origins = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        n = len(origins)
        if max_t is not None:
            max_t = np.ascontiguousarray(max_t, np.float32)
            assert max_t.shape == (n,)
        t = np.zeros(n, np.float32)
        tri = np.zeros(n, np.uint32)
        flags = np.zeros(n, np.uint32)
        self._check(lib().rpt_debug_walk_production(self._h, int(kind), n, ptr(origins), ptr(dirs), None if max_t is None else ptr(max_t), ptr(t), ptr(tri), ptr(flags)))
        return t, tri, flags


def comm_unique_id():
    """ncclGetUniqueId through the C ABI (rank 0 calls it; the 128 bytes go to every rank)."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    rc = lib().rpt_comm_unique_id(buf)
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return bytes(buf)


def device_info(device_id=0):
    """rpt_device_info: (compute units, peak engine clock in MHz) of a HIP device."""
    cus, khz = C.c_uint32(), C.c_uint32()
    rc = lib().rpt_device_info(device_id, C.byref(cus), C.byref(khz))
    if rc:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return cus.value, khz.value / 1e3


def build_fingerprint():
    """rpt_build_fingerprint: tools/source_fingerprint.py of the sources the loaded library was built from."""
    return lib().rpt_build_fingerprint().decode()


def comm_library():
    """rpt_comm_library: the collective library the process resolved ("" before the first communicator)."""
    return lib().rpt_comm_library().decode()


class MultiRenderer(_Handle):
    """rpt_multi_*: ONE process driving several GPUs (ncclCommInitAll) — the entry points a single render thread like
    the reference's (src/trace.rs:136-224) calls; the caller sees one W x H image."""
    _prefix = "rpt_multi_"

    def __init__(self, device_ids, allow_shared_device=False):
        ids = (C.c_int * len(device_ids))(*device_ids)
        self._open(lib().rpt_multi_create, ids, len(device_ids), MULTI_ALLOW_SHARED_DEVICE if allow_shared_device else 0)
        self.config = None

    def size(self):
        return lib().rpt_multi_size(self._h)

    def rank_view(self, rank):
        """The rpt_ctx of one rank as a (borrowed) Renderer: per-GPU statistics, stage times, partition queries."""
        return Renderer.borrowed(self.ctx_handle(rank), self.config, rank, self.size())

    def ctx_handle(self, rank):
        """rpt_multi_ctx: the borrowed rpt_ctx of one rank (for rpt_set_samples_in_flight / rpt_get_stats per GPU)."""
        return C.c_void_p(lib().rpt_multi_ctx(self._h, rank))

    def moments_on(self):
        return self.rank_view(0).moments_on()

    def gather_set_moments(self, on=True):
        """rpt_multi_gather_set_moments: Renderer.gather_set_moments on every rank; read_moments, denoise_variance and denoise_temporal then use the gathered
        record on rank 0 — no per-rank read-back, no host merge, no upload"""
        self._call("gather_set_moments", 1 if on else 0)

    def gather_moments(self):
        return self.rank_view(0).gather_moments()

    def gathered_info(self):
        """Renderer.gathered_info of rank 0"""
        return self.rank_view(0).gathered_info()

    def counts_uniform(self):
        """rpt_counts_uniform of every rank"""
        return all(self.rank_view(k).counts_uniform() for k in range(self.size()))

    def read_noise(self):
        """noise_host of read_moments(): the whole (H, W) image (there is no multi-GPU entry point for it: the arithmetic is the same header on the host)"""
        return noise_host(self.read_moments())[0]

    def denoise(self, params=None, tonemap_op=0, with_report=False):
        """rpt_multi_denoise: waits, gathers if need be, and denoises the whole image on rank 0 (see Renderer.denoise)"""
        return self._denoise((), params, tonemap_op, with_report)

    def denoise_variance(self, params=None, tonemap_op=0, with_report=False):
        """rpt_multi_denoise_variance: the ranks' moments merged on the host — or, after gather_set_moments(), the gathered record — the gather of denoise(),
        the filter on rank 0 (see Renderer.denoise_variance)"""
        return self._denoise_variance((), params, tonemap_op, with_report)

    def denoise_temporal(self, params=None, tonemap_op=0, with_report=False):
        """rpt_multi_denoise_temporal: as denoise_variance(); the history lives on rank 0 (see Renderer.denoise_temporal)"""
        return self._denoise_temporal((), params, tonemap_op, with_report)

    def denoise_temporal(self, params=None, tonemap_op=0, with_report=False):
        """rpt_multi_denoise_temporal: as denoise_variance(); the history lives on rank 0 (see Renderer.denoise_temporal)"""
        return self._denoise_temporal((), params, tonemap_op, with_report)

    def stats(self):
        """rpt_multi_get_stats: the counters summed over the GPUs (no times: rank_view(k).stats() has each GPU's)"""
        s = self._get_stats()
        return {k: getattr(s, k) for k in _COUNTERS}


def tile_order(width, height, rank, world_size):
    """(x | y << 16) of every pixel of `rank`'s tile-major block, in block order (no GPU needed)."""
    n = C.c_size_t()
    rc = lib().rpt_tile_order(width, height, rank, world_size, None, 0, C.byref(n))
    if rc != 0:
        raise RptError(rc, "rpt_tile_order")
    out = np.zeros(n.value, np.uint32)
    rc = lib().rpt_tile_order(width, height, rank, world_size, ptr(out), out.size, C.byref(n))
    if rc != 0:
        raise RptError(rc, "rpt_tile_order")
    return out


def lens_rays_host(config, lens, pixels_xy, keys):
    """rpt_debug_lens_rays_host: the camera rays of a configuration and a CameraLens (None: the default) for (x | y << 16, key) pairs, on the host"""
    pixels_xy, keys = np.ascontiguousarray(pixels_xy, np.uint32), np.ascontiguousarray(keys, np.uint32)
    o, d = np.zeros((len(keys), 3), np.float32), np.zeros((len(keys), 3), np.float32)
    rc = lib().rpt_debug_lens_rays_host(C.byref(config), None if lens is None else C.byref(lens), ptr(pixels_xy), ptr(keys), len(keys), ptr(o), ptr(d))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return o, d


def last_order_host(world):
    """rpt_debug_last_order_host: the upload-time decision about the order of the hit-or-miss lanes of the last extension rays, without a GPU."""
    r, n = C.c_uint32(), C.c_uint32()
    v = (C.c_double * 4)()
    flip = np.zeros(max(1, (len(world.nodes) - 1) // 2), np.uint8)
    rc = lib().rpt_debug_last_order_host(ptr(world.per_vertex), len(world.per_vertex), ptr(world.indices), len(world.indices), ptr(world.nodes), len(world.nodes),
                                         ptr(world.materials), len(world.materials), C.byref(r), v, C.byref(n), ptr(flip))
    if rc != 0:
        raise RptError(rc, "rpt_debug_last_order_host")
    return {"rule": r.value, "visits": [v[k] for k in range(4)], "probe_rays": n.value, "flip": flip}


def shadow_order_host(world):
    """rpt_debug_shadow_order_host: the upload-time decision about the shadow walks' order for a World, without a GPU."""
    f, n = C.c_uint32(), C.c_uint32()
    vn, vf = C.c_double(), C.c_double()
    flip = np.zeros(max(1, (len(world.nodes) - 1) // 2), np.uint8)
    rc = lib().rpt_debug_shadow_order_host(ptr(world.per_vertex), len(world.per_vertex), ptr(world.indices), len(world.indices), ptr(world.nodes), len(world.nodes),
                                           ptr(world.materials), len(world.materials), ptr(world.light_pick), len(world.light_pick),
                                           C.byref(f), C.byref(vn), C.byref(vf), C.byref(n), ptr(flip))
    if rc != 0:
        raise RptError(rc, "rpt_debug_shadow_order_host")
    return {"fixed": bool(f.value), "visits_near": vn.value, "visits_fixed": vf.value, "probe_rays": n.value, "flip": flip,
            "why": lib().rpt_debug_shadow_order_why(None).decode()}


def debug_math_host(op, x, y=None):
    """The host build of rpt_math.h inside librpt_hip.so (no GPU needed)."""
    x = np.ascontiguousarray(x, np.float32)
    y = x if y is None else np.ascontiguousarray(y, np.float32)
    out = np.empty_like(x)
    rc = lib().rpt_debug_math_host(op, ptr(x), ptr(y), ptr(out), x.size)
    if rc != 0:
        raise RptError(rc, "rpt_debug_math_host")
    return out


def _punctual_sample(handle, lights, q, hits, l1):
    lights = np.ascontiguousarray(lights, PUNCTUAL_LIGHT_DTYPE).reshape(-1)
    hits, l1 = np.ascontiguousarray(hits, np.float32).reshape(-1, 3), np.ascontiguousarray(l1, np.float32).reshape(-1)
    if len(hits) != len(l1):
        raise ValueError("debug_punctual_sample: one hit and one l1 per item")
    n = len(l1)
    j, L, max_t, E, pdf = np.zeros(n, np.uint32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32), np.zeros((n, 3), np.float32), np.zeros(n, np.float32)
    if handle is None:
        rc = lib().rpt_debug_punctual_sample_host(ptr(lights), len(lights), float(q), ptr(hits), ptr(l1), n, ptr(j), ptr(L), ptr(max_t), ptr(E), ptr(pdf))
    else:
        rc = lib().rpt_debug_punctual_sample(handle, ptr(lights), len(lights), float(q), ptr(hits), ptr(l1), n, ptr(j), ptr(L), ptr(max_t), ptr(E), ptr(pdf))
    if rc != 0:
        raise RptError(rc, "rpt_debug_punctual_sample")
    return j, L, max_t, E, pdf


def debug_punctual_lights_check(lights, pick_share=0.5, scene_has_emitters=True):
    """rpt_debug_punctual_lights_check (no GPU needed): what rpt_set_punctual_lights would say to these records and this share over a scene with or without
    emissive triangles -> (code, message); lights None: (NULL, 0)"""
    if lights is not None:
        lights = np.ascontiguousarray(lights, PUNCTUAL_LIGHT_DTYPE).reshape(-1)
    msg = C.create_string_buffer(512)
    rc = lib().rpt_debug_punctual_lights_check(ptr(lights), 0 if lights is None else len(lights), float(pick_share), 1 if scene_has_emitters else 0, msg, len(msg))
    return rc, msg.value.decode()


def debug_punctual_sample_host(lights, q, hits, l1):
    """The host build of csrc/k_punctual.h punctual_sample inside librpt_hip.so (no GPU needed) -> (j, L, max_t, E, pick_pdf)"""
    return _punctual_sample(None, lights, q, hits, l1)


def _volume_transmit(handle, on_device, throughput, sigma, t):
    throughput = np.ascontiguousarray(throughput, np.float32).reshape(-1, 3)
    sigma = np.ascontiguousarray(sigma, np.float32).reshape(-1, 3)
    t = np.ascontiguousarray(t, np.float32).reshape(-1)
    if not len(throughput) == len(sigma) == len(t):
        raise ValueError("debug_volume_transmit: one throughput, one sigma and one t per item")
    out = np.zeros_like(throughput)
    rc = lib().rpt_debug_volume_transmit(handle, on_device, ptr(throughput), ptr(sigma), ptr(t), len(t), ptr(out))
    if rc != 0:
        raise RptError(rc, "rpt_debug_volume_transmit")
    return out


def debug_volume_transmit_host(throughput, sigma, t):
    """The host build of csrc/k_volume.h vol_transmit inside librpt_hip.so (no GPU needed): (n, 3), (n, 3), (n,) -> (n, 3) float32"""
    return _volume_transmit(None, 0, throughput, sigma, t)


def gather_layout(width, height, world_size, with_moments=True):
    """rpt_debug_gather_layout (no GPU needed): {"stride": pixels, "slot_floats", "block_pixels": [per rank], "message_floats": [per rank]}"""
    stride, slot = C.c_uint64(), C.c_uint64()
    blocks, messages = np.zeros(world_size, np.uint64), np.zeros(world_size, np.uint64)
    rc = lib().rpt_debug_gather_layout(width, height, world_size, 1 if with_moments else 0, C.byref(stride), C.byref(slot), ptr(blocks), ptr(messages))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return {"stride": stride.value, "slot_floats": slot.value, "block_pixels": [int(b) for b in blocks], "message_floats": [int(m) for m in messages]}


def gather_host(width, height, world_size, accum_blocks, moments_blocks, trailers, slots=None):
    """rpt_debug_gather_host (no GPU needed): the ranks' blocks one behind the other ((W*H, 4) float32 each) and (world, 4) uint32 trailers through the host
    build of pack -> slots -> un-tile.  slots: None, or the landing buffer (world * slot_floats float32) as the caller initialised it, written in place.
    Returns (image (H, W, 4), moments (H, W, 4), the dictionary of gathered_info())."""
    accum_blocks, moments_blocks = np.ascontiguousarray(accum_blocks, np.float32), np.ascontiguousarray(moments_blocks, np.float32)
    trailers = np.ascontiguousarray(trailers, np.uint32)
    assert accum_blocks.size == width * height * 4 and moments_blocks.size == width * height * 4 and trailers.shape == (world_size, 4)
    assert slots is None or (slots.dtype == np.float32 and slots.flags["C_CONTIGUOUS"] and slots.size == world_size * gather_layout(width, height, world_size)["slot_floats"])
    image, moments, g = np.zeros((height, width, 4), np.float32), np.zeros((height, width, 4), np.float32), GatheredInfo()
    rc = lib().rpt_debug_gather_host(width, height, world_size, ptr(accum_blocks), ptr(moments_blocks), ptr(trailers), ptr(slots), ptr(image), ptr(moments), C.byref(g))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return image, moments, _gathered_info_dict(g)


def _report_dict(rep):
    return {"device_ms": rep.device_ms, "guides_ms": rep.guides_ms, "guides_rebuilt": rep.guides_rebuilt, "pixels_clamped": rep.pixels_clamped}


def denoise_host(mean_rgb, albedo, normal, position, depth, kind, params=None, tonemap_op=0):
    """rpt_debug_denoise_host: the filter of Renderer.denoise run on the host from the same header (no GPU needed).  mean_rgb, albedo, normal,
    position: (H, W, 3); depth, kind: (H, W) — the layouts of Renderer.guides()."""
    mean_rgb = np.ascontiguousarray(mean_rgb, np.float32)
    h, w = mean_rgb.shape[:2]
    planes = [np.ascontiguousarray(a, np.float32) for a in (albedo, normal, position, depth)]
    kind = np.ascontiguousarray(kind, np.uint32)
    assert mean_rgb.shape == (h, w, 3) and all(a.shape == (h, w, 3) for a in planes[:3]) and planes[3].shape == (h, w) and kind.shape == (h, w)
    out = np.zeros((h, w, 3), np.float32)
    rc = lib().rpt_debug_denoise_host(w, h, ptr(mean_rgb), ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), ptr(planes[3]), ptr(kind),
                                      None if params is None else C.byref(params), tonemap_op, ptr(out))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return out


def glass_step_host(world, models, max_interfaces, origins, dirs, hit_t, hit_tri, hit_flags, chain_albedo, chain_length, chain_interfaces):
    """rpt_debug_glass_step_host: one step of the chain of set_guides_through_glass for n rays, on the host from the same header (no GPU needed).  world: the
    scene's arrays (per_vertex, indices, materials, atlas or None); models: MATERIAL_MODEL_DTYPE records or None; the rays (n, 3), their nearest hits and the
    chains so far (A (n, 3), L (n), m (n)).  Nothing is changed in place: {"origins", "dirs": the next rays, "albedo_product", "length", "interfaces": the
    chains after the step, "active": the chain goes on, "kind", "normal", "albedo": the final records where it does not, "exhausted"}."""
    o, d = (np.array(a, np.float32).reshape(-1, 3) for a in (origins, dirs))
    n = len(o)
    t, tri, fl = np.ascontiguousarray(hit_t, np.float32), np.ascontiguousarray(hit_tri, np.uint32), np.ascontiguousarray(hit_flags, np.uint32)
    A, L, m = np.array(chain_albedo, np.float32).reshape(-1, 3), np.array(chain_length, np.float32).reshape(-1), np.array(chain_interfaces, np.uint32).reshape(-1)
    assert len(d) == len(t) == len(tri) == len(fl) == len(A) == len(L) == len(m) == n
    models = None if models is None else np.ascontiguousarray(models, MATERIAL_MODEL_DTYPE)
    assert models is None or len(models) == len(world.materials)
    atlas = getattr(world, "atlas", None)
    aw = ah = 0
    if atlas is not None:
        atlas = np.ascontiguousarray(atlas, np.uint8)
        ah, aw = atlas.shape[:2]
    active, exhausted, kind = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    normal, albedo = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    rc = lib().rpt_debug_glass_step_host(ptr(world.per_vertex), len(world.per_vertex), ptr(world.indices), len(world.indices), ptr(world.materials), len(world.materials),
                                         ptr(atlas), aw, ah, ptr(models), max_interfaces, n, ptr(o), ptr(d), ptr(t), ptr(tri), ptr(fl), ptr(A), ptr(L), ptr(m),
                                         ptr(active), ptr(kind), ptr(normal), ptr(albedo), ptr(exhausted))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return {"origins": o, "dirs": d, "albedo_product": A, "length": L, "interfaces": m, "active": active != 0, "kind": kind, "normal": normal, "albedo": albedo,
            "exhausted": exhausted != 0}


def denoise_variance_host(mean_rgb, albedo, normal, position, depth, kind, moments, params=None, tonemap_op=0):
    """rpt_debug_denoise_variance_host: the filter of Renderer.denoise_variance run on the host from the same headers (no GPU needed).  The planes of
    denoise_host and moments (H, W, 4) as read_moments() returns them: (rgb (H, W, 3), variance (H, W))."""
    mean_rgb = np.ascontiguousarray(mean_rgb, np.float32)
    h, w = mean_rgb.shape[:2]
    planes = [np.ascontiguousarray(a, np.float32) for a in (albedo, normal, position, depth)]
    kind, moments = np.ascontiguousarray(kind, np.uint32), np.ascontiguousarray(moments, np.float32)
    assert mean_rgb.shape == (h, w, 3) and all(a.shape == (h, w, 3) for a in planes[:3]) and planes[3].shape == (h, w) and kind.shape == (h, w) and moments.shape == (h, w, 4)
    out, var = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    rc = lib().rpt_debug_denoise_variance_host(w, h, ptr(mean_rgb), ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), ptr(planes[3]), ptr(kind), ptr(moments),
                                               None if params is None else C.byref(params), tonemap_op, ptr(out), ptr(var))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return out, var


def denoise_temporal_host(mean_rgb, albedo, normal, position, depth, kind, moments, camera, previous=None, params=None, tonemap_op=0):
    """rpt_debug_denoise_temporal_host: Renderer.denoise_temporal run on the host from the same headers (no GPU needed).  The arguments of
    denoise_variance_host, the current view's TracingConfig, and `previous`: None (no history) or {"camera": TracingConfig, "normal", "position": (H, W, 3),
    "kind": (H, W), "records": (H, W, 6) — e_h.rgb, N, mu1, mu2}.  Returns {"rgb", "variance", "history" (T), "records" (the new history: feed it to the next
    view as previous["records"]), "pixels_with_history"}."""
    mean_rgb = np.ascontiguousarray(mean_rgb, np.float32)
    h, w = mean_rgb.shape[:2]
    planes = [np.ascontiguousarray(a, np.float32) for a in (albedo, normal, position, depth)]
    kind, moments = np.ascontiguousarray(kind, np.uint32), np.ascontiguousarray(moments, np.float32)
    assert mean_rgb.shape == (h, w, 3) and all(a.shape == (h, w, 3) for a in planes[:3]) and planes[3].shape == (h, w) and kind.shape == (h, w) and moments.shape == (h, w, 4)
    prev = [None] * 5
    if previous is not None:
        prev = [C.byref(previous["camera"]), np.ascontiguousarray(previous["normal"], np.float32), np.ascontiguousarray(previous["position"], np.float32),
                np.ascontiguousarray(previous["kind"], np.uint32), np.ascontiguousarray(previous["records"], np.float32)]
        assert prev[1].shape == (h, w, 3) and prev[2].shape == (h, w, 3) and prev[3].shape == (h, w) and prev[4].shape == (h, w, 6)
    out = {"rgb": np.zeros((h, w, 3), np.float32), "variance": np.zeros((h, w), np.float32), "history": np.zeros((h, w), np.float32), "records": np.zeros((h, w, 6), np.float32)}
    count = C.c_uint64()
    rc = lib().rpt_debug_denoise_temporal_host(w, h, ptr(mean_rgb), ptr(planes[0]), ptr(planes[1]), ptr(planes[2]), ptr(planes[3]), ptr(kind), ptr(moments), C.byref(camera),
                                               prev[0], *(ptr(a) for a in prev[1:]), None if params is None else C.byref(params), tonemap_op,
                                               ptr(out["rgb"]), ptr(out["variance"]), ptr(out["history"]), ptr(out["records"]), C.byref(count))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    out["pixels_with_history"] = count.value
    return out


def firefly_host(mean_rgb, albedo, kind, moments, counts=None, samples=0, clamp_scale=2.0, clamp_floor=0.0, clamp_radius=2, demodulated=True):
    """rpt_debug_firefly_host: the firefly clamp of Renderer.denoise_variance / denoise_temporal (csrc/k_firefly.h ff_pixel) on the host from the same header
    (no GPU needed).  mean_rgb, albedo: (H, W, 3); kind: (H, W); moments: (H, W, 4); counts: (H, W) per-pixel sample counts, or None: every pixel has `samples`.
    Returns (the clamped mean (H, W, 3), the clamped records (H, W, 4), mask (H, W) uint8: 1 = clamped)."""
    mean_rgb, albedo = np.ascontiguousarray(mean_rgb, np.float32), np.ascontiguousarray(albedo, np.float32)
    h, w = mean_rgb.shape[:2]
    kind, moments = np.ascontiguousarray(kind, np.uint32), np.ascontiguousarray(moments, np.float32)
    if counts is not None:
        counts = np.ascontiguousarray(counts, np.float32)
        assert counts.shape == (h, w)
    assert mean_rgb.shape == (h, w, 3) and albedo.shape == (h, w, 3) and kind.shape == (h, w) and moments.shape == (h, w, 4)
    out, rec, mask = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 4), np.float32), np.zeros((h, w), np.uint8)
    rc = lib().rpt_debug_firefly_host(w, h, ptr(mean_rgb), ptr(albedo), ptr(kind), ptr(moments), ptr(counts), samples, clamp_scale, clamp_floor, clamp_radius,
                                      1 if demodulated else 0, ptr(out), ptr(rec), ptr(mask))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return out, rec, mask


def noise_host(moments, threshold=0.0):
    """rpt_debug_noise_host: noise_rel of every record of `moments` (..., 4) and the counts of Renderer.noise_count, on the host from the same header
    (no GPU needed): (rel with the leading shape of moments, {"pixels", "measured", "above"})"""
    moments = np.ascontiguousarray(moments, np.float32)
    assert moments.shape[-1] == 4
    rel = np.zeros(moments.shape[:-1], np.float32)
    k = NoiseCounts()
    rc = lib().rpt_debug_noise_host(ptr(moments), rel.size, threshold, ptr(rel), C.byref(k))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return rel, _counts_dict(k)


def adaptive_select_host(moments, threshold, batch_samples, max_samples):
    """rpt_debug_adaptive_select_host: the selection rule of render_adaptive over the records `moments` (..., 4) and their ordered compaction, on the host
    from the same header (no GPU needed): (flags uint8 with the leading shape of moments, the selected records' flat indices in ascending order)"""
    moments = np.ascontiguousarray(moments, np.float32)
    assert moments.shape[-1] == 4
    flags = np.zeros(moments.shape[:-1], np.uint8)
    active = np.zeros(flags.size, np.uint32)
    n = C.c_size_t()
    rc = lib().rpt_debug_adaptive_select_host(ptr(moments), flags.size, threshold, batch_samples, max_samples, ptr(flags), ptr(active), C.byref(n))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return flags, active[: n.value]


def adaptive_window_host(moments, threshold, batch_samples, max_samples, radius):
    """rpt_debug_adaptive_window_host: the window rule of render_adaptive_window over the row-major records `moments` (H, W, 4), tile by tile, on the host
    from the same header (no GPU needed): flags (H, W) uint8"""
    moments = np.ascontiguousarray(moments, np.float32)
    assert moments.ndim == 3 and moments.shape[-1] == 4
    h, w = moments.shape[:2]
    flags = np.zeros((h, w), np.uint8)
    rc = lib().rpt_debug_adaptive_window_host(ptr(moments), w, h, threshold, batch_samples, max_samples, radius, ptr(flags))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return flags


def light_table_build_gpu(vertices_xyzw, triangles, materials, device=0):
    """build_light_pick_table on the GPU (rpt_light_table_build_gpu; reference src/light_pick.rs:13-122).
    Returns (table as LIGHT_PICK_DTYPE array, number of emissive triangles, {"total", "device", "host_chains", "transfers"} in milliseconds)."""
    from ._ffi import LIGHT_PICK_DTYPE, MATERIAL_DTYPE, TRIANGLE_DTYPE
    v = np.ascontiguousarray(vertices_xyzw, np.float32).reshape(-1, 4)
    t = np.ascontiguousarray(triangles, TRIANGLE_DTYPE)
    m = np.ascontiguousarray(materials, MATERIAL_DTYPE)
    table = np.empty(max(1, len(t)), LIGHT_PICK_DTYPE)          # (np.zeros would fault in 28 bytes per triangle of pages the call overwrites)
    n, n_em = C.c_size_t(0), C.c_uint32(0)
    ms = (C.c_double * 4)()
    rc = lib().rpt_light_table_build_gpu(device, v.ctypes.data, len(v), t.ctypes.data, len(t), m.ctypes.data, len(m), table.ctypes.data, len(table),
                                         C.byref(n), C.byref(n_em), ms)
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return table[: n.value], n_em.value, {"total": ms[0], "device": ms[1], "host_chains": ms[2], "transfers": ms[3]}


def bvh_build_gpu(vertices_xyzw, triangles, sah_samples=128, device=0):
    """BVHBuilder::build on the GPU (rpt_bvh_build_gpu; reference src/bvh.rs:59-324).
    vertices_xyzw: (n, 4) float32; triangles: TRIANGLE_DTYPE array (v0, v1, v2, material).
    Returns (nodes, reordered triangles, device milliseconds)."""
    from ._ffi import BVH_NODE_DTYPE, TRIANGLE_DTYPE
    v = np.ascontiguousarray(vertices_xyzw, np.float32).reshape(-1, 4)
    # the call reorders the triangles in place: a private copy, as words (numpy copies a structured array field by field: 6 ms for 16 MB instead of 1.5)
    t = np.ascontiguousarray(triangles, TRIANGLE_DTYPE).view(np.uint32).copy().view(TRIANGLE_DTYPE)
    nodes = np.empty(max(1, 2 * len(t) - 1), BVH_NODE_DTYPE)      # (written by the call; zeroing and copying 64 MB of node pool was 25 ms of a 1 M-triangle "startup" in this harness)
    n_nodes = C.c_size_t(0)
    ms = C.c_double(0.0)
    rc = lib().rpt_bvh_build_gpu(device, v.ctypes.data, len(v), t.ctypes.data, len(t), sah_samples, nodes.ctypes.data, len(nodes),
                                 C.byref(n_nodes), C.byref(ms))
    if rc != 0:
        raise RptError(rc, lib().rpt_last_error(None).decode())
    return nodes[: n_nodes.value], t, ms.value
