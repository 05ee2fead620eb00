"""ctypes binding of libdigitalearth_hip.so (C ABI in include/digital_earth.h).

There is no CPU implementation behind this module: if the HIP library is missing, cannot be loaded, or finds no
gfx950 device, the error is raised — nothing falls back to another code path.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DE_LIB_PATH: A/B experiments load another build of the same ABI (tools/ab_build.sh) without touching the product library
LIB_PATH = os.environ.get("DE_LIB_PATH") or os.path.join(_HERE, "libdigitalearth_hip.so")


class DeParams(ctypes.Structure):
    """`de_params` (include/digital_earth.h)."""
    _fields_ = [
        ("camera_pos", ctypes.c_float * 3), ("look_at", ctypes.c_float * 3), ("up", ctypes.c_float * 3),
        ("fov", ctypes.c_float), ("aspect_scale", ctypes.c_float), ("sun_angle", ctypes.c_float),
        ("sun_path_rot", ctypes.c_float), ("land_height_scale", ctypes.c_float), ("exposure", ctypes.c_float),
        ("gamma", ctypes.c_float), ("selected_crf", ctypes.c_int32), ("vignette_strength", ctypes.c_float),
        ("vignette_radius", ctypes.c_float), ("vignette_center", ctypes.c_float * 2), ("flags", ctypes.c_uint32),
        ("fixed_wavelength", ctypes.c_float), ("topo_res_override", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7),
    ]


class DeCounters(ctypes.Structure):
    """`de_counters` (include/digital_earth.h)."""
    _fields_ = [("samples", ctypes.c_uint64), ("taps_r8", ctypes.c_uint64), ("taps_rgb8", ctypes.c_uint64),
                ("sphere_steps", ctypes.c_uint64), ("tracking_steps", ctypes.c_uint64), ("vertices", ctypes.c_uint64),
                ("rng_draws", ctypes.c_uint64), ("reserved", ctypes.c_uint64 * 9)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}
        d["sched"] = [int(x) for x in self.reserved]
        return d


class DeAdaptive(ctypes.Structure):
    """`de_adaptive` (include/digital_earth.h): the settings and the outputs of one round of an adaptive frame."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("threshold", ctypes.c_float), ("floor", ctypes.c_float),
                ("min_spp", ctypes.c_int32), ("max_spp", ctypes.c_int32), ("round_spp", ctypes.c_int32),
                ("tile_spp", ctypes.POINTER(ctypes.c_int32)), ("active_tiles", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("pixel_samples", ctypes.c_uint64)]


class DeDenoise(ctypes.Structure):
    """`de_denoise` (include/digital_earth_denoise.h): the denoiser's settings."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("levels", ctypes.c_int32), ("sigma_luminance", ctypes.c_float)]


class DeAutoExposure(ctypes.Structure):
    """`de_auto_exposure` (include/digital_earth_exposure.h): the settings of the metered exposure."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("key", ctypes.c_float), ("compensation", ctypes.c_float), ("ev_min", ctypes.c_float), ("ev_max", ctypes.c_float),
                ("low_fraction", ctypes.c_float), ("high_fraction", ctypes.c_float), ("adapt", ctypes.c_float), ("region", ctypes.c_int32 * 4)]


class DeMetering(ctypes.Structure):
    """`de_metering` (include/digital_earth_exposure.h): what the newest display metered."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("ev", ctypes.c_float), ("ev_target", ctypes.c_float), ("mean_log2", ctypes.c_float), ("valid", ctypes.c_uint32),
                ("metered", ctypes.c_uint64), ("below", ctypes.c_uint64), ("clipped", ctypes.c_uint64), ("histogram", ctypes.c_uint32 * 256)]


class DeBloom(ctypes.Structure):
    """`de_bloom` (include/digital_earth_bloom.h): the settings of the bloom."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("intensity", ctypes.c_float), ("threshold", ctypes.c_float), ("knee", ctypes.c_float), ("clamp", ctypes.c_float),
                ("spread", ctypes.c_float), ("levels", ctypes.c_int32)]


class DeHistory(ctypes.Structure):
    """`de_history` (include/digital_earth_history.h): the settings of the history reprojection."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("max_history", ctypes.c_float), ("depth_tolerance", ctypes.c_float)]


class DePixels(ctypes.Structure):
    """`de_pixels` (include/digital_earth_pixels.h): the format of the 8-bit pixel output."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("channels", ctypes.c_int32), ("mode", ctypes.c_int32), ("seed", ctypes.c_uint32), ("animate", ctypes.c_int32)]


class DeLocalExposure(ctypes.Structure):
    """`de_local_exposure` (include/digital_earth_local_exposure.h): the settings of the local exposure."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("on", ctypes.c_int32), ("highlights", ctypes.c_float), ("shadows", ctypes.c_float), ("sigma", ctypes.c_float),
                ("max_ev", ctypes.c_float), ("key", ctypes.c_float), ("levels", ctypes.c_int32)]


class DeOutputScale(ctypes.Structure):
    """`de_output_scale` (include/digital_earth_output_scale.h): the size and the filter of the resampled output."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("enabled", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("filter", ctypes.c_int32)]


class DePanorama(ctypes.Structure):
    """`de_panorama` (include/digital_earth_panorama.h): the projection, size, apron, supersampling and frame of the 360° output."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("on", ctypes.c_int32), ("projection", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("aperture_deg", ctypes.c_float), ("apron", ctypes.c_int32), ("supersample", ctypes.c_int32), ("basis", ctypes.c_float * 9)]


class DeHdrOutput(ctypes.Structure):
    """`de_hdr_output` (include/digital_earth_hdr_output.h): the HDR display output — peak luminance, gamut, transfer, and the format of its pixels."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("on", ctypes.c_int32), ("peak_nits", ctypes.c_float), ("gamut", ctypes.c_int32), ("transfer", ctypes.c_int32),
                ("pixel_format", ctypes.c_int32), ("mode", ctypes.c_int32), ("seed", ctypes.c_uint32), ("animate", ctypes.c_int32)]


class DeVideo(ctypes.Structure):
    """`de_video` (include/digital_earth_video.h): the format of the video frame output."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("format", ctypes.c_int32), ("matrix", ctypes.c_int32), ("range", ctypes.c_int32), ("siting", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("seed", ctypes.c_uint32), ("animate", ctypes.c_int32)]


class DeLook(ctypes.Structure):
    """`de_look` (include/digital_earth_look.h): the look LUTs behind the display."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("enabled", ctypes.c_int32), ("interpolation", ctypes.c_int32), ("strength", ctypes.c_float),
                ("size_1d", ctypes.c_int32), ("min_1d", ctypes.c_float * 3), ("max_1d", ctypes.c_float * 3),
                ("size_3d", ctypes.c_int32), ("min_3d", ctypes.c_float * 3), ("max_3d", ctypes.c_float * 3)]


class DeJpeg(ctypes.Structure):
    """`de_jpeg` (include/digital_earth_jpeg.h): the quality and the restart interval of the JPEG output."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("quality", ctypes.c_int32), ("restart_mcus", ctypes.c_int32)]


class DePng(ctypes.Structure):
    """`de_png` (include/digital_earth_png.h): the source, the filter and the chunk size of the PNG output."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("source", ctypes.c_int32), ("filter", ctypes.c_int32), ("chunk_bytes", ctypes.c_int32)]


class DeExr(ctypes.Structure):
    """`de_exr` (include/digital_earth_exr.h): the source, the pixel type, the compression, the chunk size and the scale of the OpenEXR output."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("source", ctypes.c_int32), ("pixel_type", ctypes.c_int32), ("compression", ctypes.c_int32),
                ("chunk_bytes", ctypes.c_int32), ("scale", ctypes.c_float)]


DE_ERR_INVALID = -1
DE_ERR_STATE = -4
DE_ERR_INTERNAL = -6
JPEG_DEFAULT_RESTART = 2      # DE_JPEG_DEFAULT_RESTART of include/digital_earth_jpeg.h
PNG_DEFAULT_CHUNK = 32768     # DE_PNG_DEFAULT_CHUNK of include/digital_earth_png.h
PNG_SOURCES = ("pixels", "hdr_pixels")                                    # DE_PNG_SOURCE_*
PNG_FILTERS = ("none", "sub", "up", "average", "paeth", "adaptive")       # DE_PNG_FILTER_*
class DeRgbe(ctypes.Structure):
    """`de_rgbe` (include/digital_earth_rgbe.h): the source, the row coding, the rounding and the scale of the Radiance HDR output."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("source", ctypes.c_int32), ("rle", ctypes.c_int32), ("rounding", ctypes.c_int32), ("scale", ctypes.c_float)]


RGBE_ROUNDINGS = {"trunc": 0, "round": 1}                                 # DE_RGBE_ROUND_TRUNC, _NEAREST
EXR_DEFAULT_CHUNK = 32768     # DE_EXR_DEFAULT_CHUNK of include/digital_earth_exr.h
EXR_SOURCES = ("mean", "denoised", "history", "bloom", "local_exposure")  # DE_EXR_SOURCE_*
EXR_PIXEL_TYPES = {"half": 1, "float": 2}                                 # DE_EXR_PIXEL_*: the file's own numbers
EXR_COMPRESSIONS = {"none": 0, "zips": 2, "zip": 3}                       # DE_EXR_COMPRESSION_*: the file's own numbers

DE_FLAG_FIXED_WAVELENGTH = 1 << 0
DE_FLAG_CLAMP_SAMPLER = 1 << 1
DE_FLAG_RAY_MARCHER = 1 << 2
DE_FLAG_AGX = 1 << 3
DE_FLAG_FAST_MATH = 1 << 5

# name -> (restype, argtypes): every symbol include/digital_earth.h declares (the binder's header)
_P = ctypes.c_void_p
SYMBOLS = {
    "de_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_P)]),
    "de_destroy": (ctypes.c_int, [_P]),
    "de_upload_texture": (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "de_generate_texture": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_int]),
    "de_share_textures": (ctypes.c_int, [_P, _P]),
    "de_trim_textures": (ctypes.c_int, [_P]),
    "de_upload_luts": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_int]),
    "de_set_params": (ctypes.c_int, [_P, ctypes.POINTER(DeParams)]),
    "de_get_params": (ctypes.c_int, [_P, ctypes.POINTER(DeParams)]),
    "de_reset": (ctypes.c_int, [_P]),
    "de_accumulate": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int]),
    "de_fetch_image": (ctypes.c_int, [_P, _P]),
    "de_fetch_image_view": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]),
    "de_fetch_image_begin": (ctypes.c_int, [_P]),
    "de_fetch_image_end": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_float))]),
    "de_render_to_image": (ctypes.c_int, [_P, ctypes.POINTER(_P)]),
    "de_fetch_hdr": (ctypes.c_int, [_P, _P]),
    "de_upload_hdr": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "de_current_spp": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int)]),
    "de_set_current_spp": (ctypes.c_int, [_P, ctypes.c_int]),
    "de_accumulate_adaptive": (ctypes.c_int, [_P, ctypes.c_uint64, ctypes.POINTER(DeAdaptive)]),
    "de_hdr_device_ptr": (ctypes.c_int, [_P, ctypes.POINTER(_P), ctypes.POINTER(ctypes.c_uint64)]),
    "de_bind_hdr": (ctypes.c_int, [_P, _P, ctypes.c_uint64]),
    "de_set_stream": (ctypes.c_int, [_P, _P]),
    "de_use_own_stream": (ctypes.c_int, [_P]),
    "de_flush": (ctypes.c_int, [_P]),
    "de_comm_unique_id": (ctypes.c_int, [_P]),
    "de_comm_init": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int]),
    "de_comm_destroy": (ctypes.c_int, [_P]),
    "de_reduce": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "de_reduce_progressive": (ctypes.c_int, [_P, _P, ctypes.c_int]),
    "de_set_sample_partition": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int]),
    "de_reduce_ordered": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int]),
    "de_set_display_source": (ctypes.c_int, [_P, _P]),
    "de_synchronize": (ctypes.c_int, [_P]),
    "de_get_tuning": (ctypes.c_int, [_P, _P]),
    "de_set_tuning": (ctypes.c_int, [_P, _P]),
    "de_last_error": (ctypes.c_char_p, []),
    "de_abi_version": (ctypes.c_int, []),
    "de_arithmetic_contract": (ctypes.c_int, []),
}

# measurement, experiment and test hooks: include/digital_earth_debug.h (same library)
DEBUG_SYMBOLS = {
    "de_download_texture": (ctypes.c_int, [_P, ctypes.c_int, _P, ctypes.c_uint64]),
    "de_debug_adaptive_moments": (ctypes.c_int, [_P, _P]),
    "de_debug_denoise": (ctypes.c_int, [_P, _P, _P, _P, ctypes.c_int, ctypes.c_float, _P]),
    "de_debug_history": (ctypes.c_int, [_P, _P, _P, _P, ctypes.POINTER(DeParams), _P, _P, ctypes.POINTER(DeParams), ctypes.c_float, ctypes.c_float, _P]),
    "de_debug_pixels": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DePixels), ctypes.c_uint32, _P]),
    "de_debug_output_scale": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DeOutputScale), _P]),
    "de_debug_output_scale_weights": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.POINTER(ctypes.c_int)]),
    "de_debug_panorama": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.POINTER(DePanorama), _P]),
    "de_debug_hdr_consts": (ctypes.c_int, [_P, ctypes.POINTER(DeHdrOutput), _P]),
    "de_texture_info": (ctypes.c_int, [_P, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 3),
    "de_last_reduce_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "de_set_launch_slots": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int]),
    "de_set_wave_budget": (ctypes.c_int, [_P, ctypes.c_int]),
    "de_last_accumulate_ms": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "de_get_counters": (ctypes.c_int, [_P, ctypes.POINTER(DeCounters)]),
    "de_enable_counters": (ctypes.c_int, [_P, ctypes.c_int]),
    "de_set_kernel_variant": (ctypes.c_int, [_P, ctypes.c_int]),
    "de_debug_samples": (ctypes.c_int, [_P, ctypes.c_uint64, ctypes.c_int, _P]),
    "de_debug_sched_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "de_set_memory_budget": (ctypes.c_int, [_P, ctypes.c_uint64]),
    "de_get_memory_use": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64)]),
    "de_last_call_info": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "de_last_launch_phases": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_float)]),
    "de_debug_v6_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
    "de_debug_cloud_bound": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_uint32)]),
    "de_debug_math": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P, ctypes.c_uint64]),
    "de_debug_math_fast": (ctypes.c_int, [_P, ctypes.c_int, _P, _P, _P, ctypes.c_uint64]),
    "de_debug_ordered_sum": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P]),
    "de_debug_standin_reduce": (ctypes.c_int, [_P, ctypes.c_int]),
}

# the denoiser: include/digital_earth_denoise.h (same library, additions only; not part of the binder's header)
DENOISE_SYMBOLS = {
    "de_set_denoise": (ctypes.c_int, [_P, ctypes.POINTER(DeDenoise)]),
    "de_get_denoise": (ctypes.c_int, [_P, ctypes.POINTER(DeDenoise)]),
    "de_fetch_denoised_hdr": (ctypes.c_int, [_P, _P]),
    "de_fetch_guides": (ctypes.c_int, [_P, _P]),
}

# auto-exposure: include/digital_earth_exposure.h (same library, additions only; not part of the binder's header)
EXPOSURE_SYMBOLS = {
    "de_set_auto_exposure": (ctypes.c_int, [_P, ctypes.POINTER(DeAutoExposure)]),
    "de_get_auto_exposure": (ctypes.c_int, [_P, ctypes.POINTER(DeAutoExposure)]),
    "de_get_metering": (ctypes.c_int, [_P, ctypes.POINTER(DeMetering)]),
}

# bloom: include/digital_earth_bloom.h (same library, additions only; not part of the binder's header)
BLOOM_SYMBOLS = {
    "de_set_bloom": (ctypes.c_int, [_P, ctypes.POINTER(DeBloom)]),
    "de_get_bloom": (ctypes.c_int, [_P, ctypes.POINTER(DeBloom)]),
    "de_fetch_bloom_hdr": (ctypes.c_int, [_P, _P]),
}

# history reprojection: include/digital_earth_history.h (same library, additions only; not part of the binder's header)
HISTORY_SYMBOLS = {
    "de_set_history": (ctypes.c_int, [_P, ctypes.POINTER(DeHistory)]),
    "de_get_history": (ctypes.c_int, [_P, ctypes.POINTER(DeHistory)]),
    "de_fetch_history_hdr": (ctypes.c_int, [_P, _P]),
}

# 8-bit pixel output: include/digital_earth_pixels.h (same library, additions only; not part of the binder's header)
PIXELS_SYMBOLS = {
    "de_set_pixels": (ctypes.c_int, [_P, ctypes.POINTER(DePixels)]),
    "de_get_pixels": (ctypes.c_int, [_P, ctypes.POINTER(DePixels), ctypes.POINTER(ctypes.c_uint32)]),
    "de_render_to_pixels": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_void_p)]),
    "de_fetch_pixels": (ctypes.c_int, [_P, _P, ctypes.c_uint64]),
    "de_fetch_pixels_view": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))]),
    "de_fetch_pixels_begin": (ctypes.c_int, [_P]),
    "de_fetch_pixels_end": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))]),
}

# local exposure: include/digital_earth_local_exposure.h (same library, additions only; not part of the binder's header)
LOCAL_EXPOSURE_SYMBOLS = {
    "de_set_local_exposure": (ctypes.c_int, [_P, ctypes.POINTER(DeLocalExposure)]),
    "de_get_local_exposure": (ctypes.c_int, [_P, ctypes.POINTER(DeLocalExposure)]),
    "de_fetch_local_exposure_hdr": (ctypes.c_int, [_P, _P]),
    "de_debug_local_exposure": (ctypes.c_int, [_P, _P, ctypes.c_float, ctypes.POINTER(DeLocalExposure), _P]),
}

# output scaling: include/digital_earth_output_scale.h (same library, additions only; not part of the binder's header)
OUTPUT_SCALE_SYMBOLS = {
    "de_set_output_scale": (ctypes.c_int, [_P, ctypes.POINTER(DeOutputScale)]),
    "de_get_output_scale": (ctypes.c_int, [_P, ctypes.POINTER(DeOutputScale)]),
    "de_output_size": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
}

# panorama output: include/digital_earth_panorama.h (same library, additions only; not part of the binder's header)
_F3 = ctypes.POINTER(ctypes.c_float)
PANORAMA_SYMBOLS = {
    "de_set_panorama": (ctypes.c_int, [_P, ctypes.POINTER(DePanorama)]),
    "de_get_panorama": (ctypes.c_int, [_P, ctypes.POINTER(DePanorama)]),
    "de_panorama_face_camera": (ctypes.c_int, [_P, ctypes.c_int, _F3, _F3, _F3, _F3]),
    "de_panorama_capture": (ctypes.c_int, [_P, ctypes.c_int]),
    "de_panorama_captured": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint32)]),
}

# scene-linear panorama: include/digital_earth_environment.h (same library, additions only; not part of the binder's header)
ENVIRONMENT_SYMBOLS = {
    "de_environment_capture": (ctypes.c_int, [_P, ctypes.c_int]),
    "de_environment_captured": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint32)]),
    "de_fetch_environment_face": (ctypes.c_int, [_P, ctypes.c_int, _P]),
    "de_debug_environment_exr": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.POINTER(DePanorama), ctypes.POINTER(DeExr), _P, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)]),
}

# HDR display output: include/digital_earth_hdr_output.h (same library, additions only; not part of the binder's header)
HDR_OUTPUT_SYMBOLS = {
    "de_set_hdr_output": (ctypes.c_int, [_P, ctypes.POINTER(DeHdrOutput)]),
    "de_get_hdr_output": (ctypes.c_int, [_P, ctypes.POINTER(DeHdrOutput), ctypes.POINTER(ctypes.c_uint32)]),
    "de_render_to_hdr_pixels": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_void_p)]),
    "de_fetch_hdr_pixels": (ctypes.c_int, [_P, _P, ctypes.c_uint64]),
    "de_debug_hdr_transform": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.POINTER(DeHdrOutput), _P]),
}

# video frame output: include/digital_earth_video.h (same library, additions only; not part of the binder's header)
VIDEO_SYMBOLS = {
    "de_set_video": (ctypes.c_int, [_P, ctypes.POINTER(DeVideo)]),
    "de_get_video": (ctypes.c_int, [_P, ctypes.POINTER(DeVideo), ctypes.POINTER(ctypes.c_uint32)]),
    "de_videoframe_bytes": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    "de_render_to_video": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_void_p)]),
    "de_fetch_video": (ctypes.c_int, [_P, _P, ctypes.c_uint64]),
    "de_fetch_videoframe_view": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))]),
    "de_fetch_videoframe_begin": (ctypes.c_int, [_P]),
    "de_fetch_videoframe_end": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8))]),
    "de_debug_video": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DeVideo), ctypes.c_uint32, _P]),
}

# JPEG output: include/digital_earth_jpeg.h (same library, additions only; not part of the binder's header)
_U64P = ctypes.POINTER(ctypes.c_uint64)
JPEG_SYMBOLS = {
    "de_set_jpeg": (ctypes.c_int, [_P, ctypes.POINTER(DeJpeg)]),
    "de_get_jpeg": (ctypes.c_int, [_P, ctypes.POINTER(DeJpeg)]),
    "de_jpeg_capacity": (ctypes.c_int, [_P, _U64P]),
    "de_render_to_jpeg": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "de_fetch_jpeg": (ctypes.c_int, [_P, _P, ctypes.c_uint64, _U64P]),
    "de_fetch_jpeg_view": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), _U64P]),
    "de_fetch_jpeg_begin": (ctypes.c_int, [_P]),
    "de_fetch_jpeg_end": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), _U64P]),
    "de_debug_jpeg": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DeJpeg), _P, ctypes.c_uint64, _U64P]),
    "de_debug_jpeg_framing": (ctypes.c_int, [ctypes.POINTER(DeJpeg), ctypes.c_int, ctypes.c_int, _P, ctypes.c_uint64, _U64P, _U64P]),
}

# PNG output: include/digital_earth_png.h (same library, additions only; not part of the binder's header)
PNG_SYMBOLS = {
    "de_set_png": (ctypes.c_int, [_P, ctypes.POINTER(DePng)]),
    "de_get_png": (ctypes.c_int, [_P, ctypes.POINTER(DePng)]),
    "de_png_capacity": (ctypes.c_int, [_P, _U64P]),
    "de_render_to_png": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "de_fetch_png": (ctypes.c_int, [_P, _P, ctypes.c_uint64, _U64P]),
    "de_fetch_png_view": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), _U64P]),
    "de_fetch_png_begin": (ctypes.c_int, [_P]),
    "de_fetch_png_end": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), _U64P]),
    "de_debug_png": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DePng), _P, ctypes.c_uint64, _U64P]),
    "de_debug_png_framing": (ctypes.c_int, [ctypes.POINTER(DePng), ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, _P, _P, ctypes.c_uint64, _U64P, _U64P]),
}
# EXR AOV channels: include/digital_earth_exr_aovs.h (same library, additions only; not part of the binder's header)
EXR_AOVS = {"depth": 1, "normal": 2, "albedo": 4, "coverage": 8, "transmittance": 16, "variance": 32, "samples": 64}      # DE_EXR_AOV_*
EXR_AOV_ALL = 127
EXR_AOV_SYMBOLS = {
    "de_set_exr_aovs": (ctypes.c_int, [_P, ctypes.c_uint32]),
    "de_get_exr_aovs": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint32)]),
    "de_debug_exr_aovs": (ctypes.c_int, [_P, _P, _P, _P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DeExr), ctypes.c_uint32, _P, ctypes.c_uint64, _U64P]),
    "de_debug_exr_aov_framing": (ctypes.c_int, [ctypes.POINTER(DeExr), ctypes.c_uint32, ctypes.c_int, ctypes.c_int, _P, ctypes.c_uint64, _U64P, _U64P]),
}
# OpenEXR output: include/digital_earth_exr.h (same library, additions only; not part of the binder's header)
EXR_SYMBOLS = {
    "de_set_exr": (ctypes.c_int, [_P, ctypes.POINTER(DeExr)]),
    "de_get_exr": (ctypes.c_int, [_P, ctypes.POINTER(DeExr)]),
    "de_exr_capacity": (ctypes.c_int, [_P, _U64P]),
    "de_render_to_exr": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "de_fetch_exr": (ctypes.c_int, [_P, _P, ctypes.c_uint64, _U64P]),
    "de_fetch_exr_view": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), _U64P]),
    "de_fetch_exr_begin": (ctypes.c_int, [_P]),
    "de_fetch_exr_end": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), _U64P]),
    "de_debug_exr": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DeExr), _P, ctypes.c_uint64, _U64P]),
    "de_debug_exr_framing": (ctypes.c_int, [ctypes.POINTER(DeExr), ctypes.c_int, ctypes.c_int, _P, ctypes.c_uint64, _U64P, _U64P]),
}

# Radiance HDR output: include/digital_earth_rgbe.h (same library, additions only; not part of the binder's header)
RGBE_SYMBOLS = {
    "de_set_rgbe": (ctypes.c_int, [_P, ctypes.POINTER(DeRgbe)]),
    "de_get_rgbe": (ctypes.c_int, [_P, ctypes.POINTER(DeRgbe)]),
    "de_rgbe_capacity": (ctypes.c_int, [_P, _U64P]),
    "de_render_to_rgbe": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p)]),
    "de_fetch_rgbe": (ctypes.c_int, [_P, _P, ctypes.c_uint64, _U64P]),
    "de_fetch_rgbe_view": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), _U64P]),
    "de_fetch_rgbe_begin": (ctypes.c_int, [_P]),
    "de_fetch_rgbe_end": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)), _U64P]),
    "de_debug_rgbe": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DeRgbe), _P, ctypes.c_uint64, _U64P]),
    "de_debug_rgbe_framing": (ctypes.c_int, [ctypes.POINTER(DeRgbe), ctypes.c_int, ctypes.c_int, _P, ctypes.c_uint64, _U64P, _U64P]),
    "de_debug_environment_rgbe": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.POINTER(DePanorama), ctypes.POINTER(DeRgbe), _P, ctypes.c_uint64, _U64P]),
}


class DeIbl(ctypes.Structure):
    """`de_ibl` (include/digital_earth_ibl.h): the cube edge, the specular levels, the samples per texel, the base level's supersample, the level-of-detail
    bias and the DDS file's pixel type."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("edge", ctypes.c_int32), ("levels", ctypes.c_int32), ("samples", ctypes.c_int32),
                ("supersample", ctypes.c_int32), ("lod_bias", ctypes.c_float), ("pixel_type", ctypes.c_int32)]


# IBL output: include/digital_earth_ibl.h (same library, additions only; not part of the binder's header)
IBL_SYMBOLS = {
    "de_set_ibl": (ctypes.c_int, [_P, ctypes.POINTER(DeIbl)]),
    "de_get_ibl": (ctypes.c_int, [_P, ctypes.POINTER(DeIbl)]),
    "de_ibl_build": (ctypes.c_int, [_P]),
    "de_fetch_ibl_sh": (ctypes.c_int, [_P, _P]),
    "de_fetch_ibl_face": (ctypes.c_int, [_P, ctypes.c_int, ctypes.c_int, _P]),
    "de_ibl_file_bytes": (ctypes.c_int, [_P, _U64P]),
    "de_fetch_ibl_dds": (ctypes.c_int, [_P, _P, ctypes.c_uint64]),
    "de_debug_ibl": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.POINTER(DePanorama), ctypes.POINTER(DeIbl), _P, _P, _P, ctypes.c_uint64]),
}

class DeIblBc6h(ctypes.Structure):
    """`de_ibl_bc6h` (include/digital_earth_ibl_bc6h.h): the BC6H stage of the IBL output, off by default, and its quality 0 or 1."""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("on", ctypes.c_int32), ("quality", ctypes.c_int32)]


# IBL output, BC6H-compressed: include/digital_earth_ibl_bc6h.h (same library, additions only; not part of the binder's header)
IBL_BC6H_SYMBOLS = {
    "de_set_ibl_bc6h": (ctypes.c_int, [_P, ctypes.POINTER(DeIblBc6h)]),
    "de_get_ibl_bc6h": (ctypes.c_int, [_P, ctypes.POINTER(DeIblBc6h)]),
    "de_ibl_bc6h_file_bytes": (ctypes.c_int, [_P, _U64P]),
    "de_fetch_ibl_bc6h_dds": (ctypes.c_int, [_P, _P, ctypes.c_uint64]),
    "de_debug_bc6h_encode": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(DeIblBc6h), _P, ctypes.c_uint64]),
    "de_debug_ibl_bc6h": (ctypes.c_int, [_P, _P, ctypes.c_int, ctypes.POINTER(DePanorama), ctypes.POINTER(DeIbl), ctypes.POINTER(DeIblBc6h), _P, _P, _P, _P, ctypes.c_uint64]),
}

# look LUTs: include/digital_earth_look.h (same library, additions only; not part of the binder's header)
LOOK_SYMBOLS = {
    "de_set_look": (ctypes.c_int, [_P, ctypes.POINTER(DeLook), _P, _P]),
    "de_get_look": (ctypes.c_int, [_P, ctypes.POINTER(DeLook)]),
    "de_debug_look": (ctypes.c_int, [_P, _P, ctypes.c_uint64, ctypes.POINTER(DeLook), _P, _P, _P]),
}

# entry points of the legacy library only (include/digital_earth_legacy.h): bound when present
LEGACY_SYMBOLS = {
    "de_debug_v5_stats": (ctypes.c_int, [_P, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]),
}


class DeTuning(ctypes.Structure):
    """de_tuning of include/digital_earth.h"""
    _fields_ = [("struct_bytes", ctypes.c_uint32), ("kernel_variant", ctypes.c_int32), ("launch_slots", ctypes.c_int32), ("big_launch_slots", ctypes.c_int32),
                ("v6_min_paths", ctypes.c_uint64), ("v6_service_area", ctypes.c_int32 * 3), ("v6_service_lanes", ctypes.c_int32 * 3),
                ("v6_yield_max", ctypes.c_int32), ("v6_elsewhere_min", ctypes.c_int32), ("v6_retry", ctypes.c_int32), ("v6_enter_min", ctypes.c_int32),
                ("v6_flat_min", ctypes.c_int32), ("v6_flat_again", ctypes.c_int32), ("v6_bands", ctypes.c_int32),
                ("v6_tail_levels", ctypes.c_int32), ("v6_tail_export", ctypes.c_int32 * 2), ("v6_tail_min_paths", ctypes.c_uint32), ("v6_tail_when_alone", ctypes.c_int32), ("v6_tail_grid", ctypes.c_int32 * 2), ("v6_stats", ctypes.c_int32),
                ("v2_pend", ctypes.c_int32), ("v2_heavy", ctypes.c_int32), ("v2_b", ctypes.c_int32), ("v2_gas", ctypes.c_int32), ("v2_chunk", ctypes.c_int32),
                ("v2_waves_per_cu", ctypes.c_int32), ("v2_max_spp", ctypes.c_int32), ("trace", ctypes.c_int32), ("v6_cu_withhold", ctypes.c_int32)]


# Experiment overrides: the LIBRARY reads no environment variable for its tuning (de_set_tuning); this layer does, once per context, for the
# tools and tests that sweep knobs from the shell.  environment name -> (de_tuning field, index or None)
ENV_TUNING = {
    "DE_KERNEL": ("kernel_variant", None), "DE_SLOTS": ("launch_slots", None), "DE_BIG_SLOTS": ("big_launch_slots", None),
    "DE_AUTO_V6_MIN_ITEMS": ("v6_min_paths", None), "DE_V6_STATS": ("v6_stats", None), "DE_AUTO_TRACE": ("trace", None),
    "DE_V6_AREA_ST": ("v6_service_area", 0), "DE_V6_AREA_GAS": ("v6_service_area", 1), "DE_V6_AREA_CLOUD": ("v6_service_area", 2),
    "DE_V6_SVC_ST": ("v6_service_lanes", 0), "DE_V6_SVC_GAS": ("v6_service_lanes", 1), "DE_V6_SVC_CLOUD": ("v6_service_lanes", 2),
    "DE_V6_YIELD": ("v6_yield_max", None), "DE_V6_ELSEWHERE": ("v6_elsewhere_min", None), "DE_V6_RETRY": ("v6_retry", None),
    "DE_V6_ENTER_MIN": ("v6_enter_min", None), "DE_V6_FLAT_MIN": ("v6_flat_min", None), "DE_V6_FLAT_AGAIN": ("v6_flat_again", None), "DE_V6_BANDS": ("v6_bands", None),
    "DE_V6_TAIL": ("v6_tail_levels", None), "DE_V6_TAIL_EXPORT0": ("v6_tail_export", 0), "DE_V6_TAIL_EXPORT1": ("v6_tail_export", 1),
    "DE_V6_TAIL_MIN_PATHS": ("v6_tail_min_paths", None), "DE_V6_TAIL_ALONE": ("v6_tail_when_alone", None), "DE_V6_TAIL_GRID0": ("v6_tail_grid", 0), "DE_V6_TAIL_GRID1": ("v6_tail_grid", 1),
    "DE_V2_THR": ("v2_pend", None), "DE_V2_A": ("v2_heavy", None), "DE_V2_B": ("v2_b", None), "DE_V2_G": ("v2_gas", None),
    "DE_V6_CU_WITHHOLD": ("v6_cu_withhold", None), "DE_V2_CHUNK": ("v2_chunk", None), "DE_V2_WPC": ("v2_waves_per_cu", None), "DE_V2_MAX_SPP": ("v2_max_spp", None),
}


def apply_env_tuning(handle):
    """Read the experiment overrides above from the environment and hand them to the context in one de_set_tuning call (nothing is set: no call)."""
    found = {k: os.environ[k] for k in ENV_TUNING if os.environ.get(k, "") != ""}
    if not found:
        return
    L = load()
    t = DeTuning()
    check(L.de_get_tuning(handle, ctypes.byref(t)))
    for name, text in found.items():
        field, i = ENV_TUNING[name]
        value = 1 if (name == "DE_AUTO_TRACE" and not text.lstrip("-").isdigit()) else int(text)
        if i is None:
            setattr(t, field, value)
        else:
            getattr(t, field)[i] = value
    if "DE_SLOTS" in found and "DE_BIG_SLOTS" not in found:
        t.big_launch_slots = min(t.big_launch_slots, t.launch_slots)
    check(L.de_set_tuning(handle, ctypes.byref(t)))


_lib = None
ABI_VERSION = 6   # DE_ABI_VERSION of include/digital_earth.h


class NativeLibraryError(RuntimeError):
    pass


def load():
    """Load libdigitalearth_hip.so and type every entry point.  Raises NativeLibraryError if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    # The launch slots of a context (de_accumulate) are HIP streams; the runtime multiplexes streams onto GPU_MAX_HW_QUEUES
    # hardware queues (default 4) and launches that share a queue run one after the other.  16 queues let the 8 slots of a
    # context run side by side (measured, tools/one_spp.py: 64 x accumulate(1) takes 2.3x the time of accumulate(64) with 4
    # queues, 1.3x with 16).  Only a default: an exported value wins, and it has no effect once HIP is initialised.
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
    if not os.path.exists(LIB_PATH):
        raise NativeLibraryError(
            "%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback." % LIB_PATH)
    try:
        L = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise NativeLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    for name, (res, args) in list(SYMBOLS.items()) + list(DEBUG_SYMBOLS.items()) + list(DENOISE_SYMBOLS.items()) + list(EXPOSURE_SYMBOLS.items()) + list(BLOOM_SYMBOLS.items()) + list(HISTORY_SYMBOLS.items()) + list(PIXELS_SYMBOLS.items()) + list(LOCAL_EXPOSURE_SYMBOLS.items()) + list(OUTPUT_SCALE_SYMBOLS.items()) + list(HDR_OUTPUT_SYMBOLS.items()) + list(VIDEO_SYMBOLS.items()) + list(LOOK_SYMBOLS.items()) + list(JPEG_SYMBOLS.items()) + list(PNG_SYMBOLS.items()) + list(EXR_SYMBOLS.items()) + list(EXR_AOV_SYMBOLS.items()) + list(PANORAMA_SYMBOLS.items()) + list(ENVIRONMENT_SYMBOLS.items()) + list(RGBE_SYMBOLS.items()) + list(IBL_SYMBOLS.items()) + list(IBL_BC6H_SYMBOLS.items()):
        try:
            fn = getattr(L, name)
        except AttributeError:
            raise NativeLibraryError("%s does not export %s" % (LIB_PATH, name))
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in LEGACY_SYMBOLS.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
    if L.de_abi_version() != ABI_VERSION:
        raise NativeLibraryError("%s has ABI version %d, this binding expects %d: rebuild it" % (LIB_PATH, L.de_abi_version(), ABI_VERSION))
    _lib = L
    return L


class DigitalEarthError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "libdigitalearth_hip error %d: %s" % (code, message))
        self.code = code


def check(rc):
    if rc != 0:
        raise DigitalEarthError(rc, load().de_last_error().decode(errors="replace"))
