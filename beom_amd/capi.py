"""ctypes binding of the C-ABI declared in include/beom_hip.h (libbeom_hip.so).

This is the Python host's FFI stub — the same calls the Fortran host makes through
iso_c_binding (beom_amd/host/beom_cabi.f95).  There is no fallback: if the HIP
library is missing or no GPU is usable, `load()`/`Engine()` raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

from .grid import Fields
from .params import Params

BEOM_MAX_LAYERS = 16
BEOM_ABI_VERSION = 2
BEOM_MAX_TRACERS = 8
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BEOM_HIP_LIB", os.path.join(_HERE, "csrc", "libbeom_hip.so"))


class BeomParams(C.Structure):
    """struct beom_params of include/beom_hip.h."""
    _fields_ = (
        [(n, C.c_int32) for n in ("abi_version", "lm", "mm", "nlay", "ndeg", "nsal", "variant",
                                  "flag_nudging", "dense_hint", "slab_row0", "slab_mm")]
        + [(n, C.c_double) for n in ("dl", "dt", "grav", "rho0", "beta", "epsi", "gamm", "del1",
                                     "del2", "hmin", "hsal", "bvis", "dvis", "svis", "bdrg",
                                     "tdrg", "qdrg", "hsbl", "hbbl", "g_fb", "uadv", "ocrp",
                                     "rgld", "mcbc", "invf", "w_ti")]
        + [("rhon", C.c_double * BEOM_MAX_LAYERS)]
    )


STATICS_NAMES = ("fcor", "h_th", "h_to", "nudg", "fnud", "hdot", "tide", "bodf", "taus")


class BeomStatics(C.Structure):
    """struct beom_statics of include/beom_hip.h."""
    _fields_ = [(n, C.POINTER(C.c_double)) for n in STATICS_NAMES]


class BeomState(C.Structure):
    """struct beom_state of include/beom_hip.h."""
    _fields_ = [(n, C.POINTER(C.c_double)) for n in ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy",
                                                     "v_cc", "v_ll", "tt3d", "tb3d", "tu3d")]


XCHG_PEER, XCHG_RCCL, XCHG_SHM, XCHG_RING1, XCHG_LOOPBACK = 0, 1, 2, 0x100, 0x200


def make_params_struct(p: Params, f: Optional[Fields] = None, variant: int = 0,
                       dense_hint: int = 1, slab_row0: int = 0, slab_mm: int = 0) -> BeomParams:
    s = BeomParams()
    s.abi_version = BEOM_ABI_VERSION
    s.lm, s.mm, s.nlay, s.ndeg = p.lm, p.mm, p.nlay, p.ndeg
    s.nsal = p.nsal
    s.variant = variant
    s.flag_nudging = int(bool(f.flag_nudging)) if f is not None else 0
    s.dense_hint = dense_hint
    s.slab_row0, s.slab_mm = slab_row0, slab_mm
    for n in ("dl", "dt", "grav", "rho0", "beta", "epsi", "gamm", "del1", "del2", "hmin", "hsal",
              "bvis", "dvis", "svis", "bdrg", "tdrg", "qdrg", "hsbl", "hbbl", "g_fb", "uadv",
              "ocrp", "rgld", "mcbc"):
        setattr(s, n, float(getattr(p, n)))
    s.invf = float(f.invf) if f is not None else 0.0
    s.w_ti = float(f.w_ti[0]) if f is not None else 0.0
    if p.nlay > BEOM_MAX_LAYERS:
        raise ValueError("nlay > BEOM_MAX_LAYERS")
    for i, r in enumerate(p.rhon_v):
        s.rhon[i] = float(r)
    return s


def _dp(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"], (a.dtype, a.flags)
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(C.POINTER(C.c_int32))


_lib = None
ERRLEN = 999                       # lstr of shared_mod.f95:34


def source_hash() -> str:
    """The hash the Makefile embeds: sha1 of the library's sources in the Makefile's order."""
    import hashlib
    csrc = os.path.join(_HERE, "csrc")
    h = hashlib.sha1()
    for fn in ("beom_engine.hip", "beom_multi.hip", "beom_dev.h", "beom_kernels.h", "beom_integrals.h", "beom_series.h", "beom_tracers.h", "beom_tracers_lim.h", "beom_tracer_mix.h", "beom_tracer_vmix.h", "beom_floats.h", "beom_moments.h", "beom_harmonics.h", "beom_tracer_moments.h", "beom_tracer_series.h", "beom_forcing.h", "beom_dense_host.h",
               "beom_bands_host.h", "beom_plan.h", "beom_recorder.h", "beom_column_series.h", "beom_tracer_column_series.h", "beom_maps.h", os.path.join("..", "..", "include", "beom_hip.h")):
        with open(os.path.join(csrc, fn), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def load(path: Optional[str] = None) -> C.CDLL:
    """Loads libbeom_hip.so and declares every prototype of include/beom_hip.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64, and if this
    # library pulls in /opt/rocm's copy first, torch later finds "No HIP GPUs".  Let torch
    # (when present) load its runtime first; libbeom_hip.so then binds to the same one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(path):
        raise RuntimeError("HIP engine library %s not built (run __graft_entry__.build()); "
                           "there is no CPU fallback" % path)
    lib = C.CDLL(path)
    if path == LIB_PATH and os.environ.get("BEOM_HIP_LIB") is None:      # in-tree library: must match the in-tree sources
        lib.beom_source_hash.restype = C.c_char_p
        built, tree = lib.beom_source_hash().decode(), source_hash()
        if built != tree:
            raise RuntimeError("libbeom_hip.so was built from other sources (%s, tree %s): run "
                               "__graft_entry__.build()" % (built, tree))
    dpp, ipp, cp, ci, cd = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_char_p, C.c_int, C.c_double
    H = C.c_void_p
    lib.beom_abi_version.restype = ci
    lib.beom_device_count.argtypes = [cp, ci]
    lib.beom_device_pci_bus_id.argtypes = [ci, cp, ci]
    lib.beom_device_pci_bus_id.restype = ci
    lib.beom_create.argtypes = [C.POINTER(BeomParams), ci, ipp, ipp] + [dpp] * 14 + [C.POINTER(H), cp, ci]
    lib.beom_destroy.argtypes = [H]
    lib.beom_set_rigid_lid.argtypes = [H, dpp, dpp, dpp, dpp, cp, ci]
    lib.beom_download_pressure.argtypes = [H, dpp, cp, ci]
    lib.beom_upload_state.argtypes = [H] + [dpp] * 13 + [cp, ci]
    lib.beom_download_state.argtypes = [H] + [dpp] * 13 + [cp, ci]
    lib.beom_download_scratch.argtypes = [H] + [dpp] * 6 + [cp, ci]
    lib.beom_step.argtypes = [H, ci, ci, cd, cd, cd, cd, ci, cp, ci]
    lib.beom_sync.argtypes = [H, cp, ci]
    lib.beom_set_stream.argtypes = [H, C.c_void_p, ci]
    lib.beom_set_option.argtypes = [H, cp, ci]
    lib.beom_set_open_boundaries.argtypes = [H, ci, ipp, cp, ci]
    lib.beom_multi_set_open_boundaries.argtypes = [H, ci, ipp, cp, ci]
    lib.beom_download_outputs.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, dpp, C.POINTER(ci), cp, ci]
    lib.beom_download_diag.argtypes = [H, C.c_void_p, C.c_void_p, C.c_void_p, cp, ci]
    lib.beom_download_diag.restype = ci
    lib.beom_step_phase.argtypes = [H, ci, cd, cd, cd, cd, ci, ci, cp, ci]
    lib.beom_pack_rows.argtypes = [H, ci, ci, C.c_void_p]
    lib.beom_unpack_rows.argtypes = [H, ci, ci, C.c_void_p]
    lib.beom_pack_rows2.argtypes = [H, ci, ci, C.c_void_p, ci, C.c_void_p]
    lib.beom_unpack_rows2.argtypes = [H, ci, ci, C.c_void_p, ci, C.c_void_p]
    lib.beom_profile_start.argtypes = [H]
    lib.beom_profile_stop.argtypes = [H, dpp, C.POINTER(ci), cp, ci]
    lib.beom_update_h.argtypes = [H, cd, cd, cd]
    lib.beom_update_mont_rvor_pvor_dive_kine.argtypes = [H, ci]
    lib.beom_update_viscosity.argtypes = [H, ci]
    lib.beom_update_u.argtypes = [H, ci, cd, cd, cd]
    lib.beom_update_v.argtypes = [H, ci, cd, cd, cd]
    lib.beom_rebuild_fluxes.argtypes = [H]
    lib.beom_distribute_stress.argtypes = [H]
    lib.beom_info.argtypes = [H, cp]
    lib.beom_info.restype = ci
    lib.beom_device_field.argtypes = [H, cp, C.POINTER(C.c_void_p), C.POINTER(C.c_int64),
                                      C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.beom_is_dense.argtypes = [H]
    lib.beom_profile_steps.argtypes = [H, ci, ci, cd, cd, cd, cd, ci, dpp, C.POINTER(ci), cp, ci]
    MH = C.c_void_p
    lib.beom_multi_create.argtypes = [C.POINTER(BeomParams), ci, C.POINTER(ci), ipp, ipp] + [dpp] * 14 + [C.POINTER(MH), cp, ci]
    lib.beom_multi_destroy.argtypes = [MH]
    lib.beom_multi_count.argtypes = [MH]
    lib.beom_multi_band.argtypes = [MH, ci] + [C.POINTER(ci)] * 5
    lib.beom_multi_upload_state.argtypes = [MH] + [dpp] * 13 + [cp, ci]
    lib.beom_multi_download_state.argtypes = [MH] + [dpp] * 13 + [cp, ci]
    lib.beom_multi_step.argtypes = [MH, ci, ci, cd, cd, cd, cd, ci, cp, ci]
    lib.beom_multi_sync.argtypes = [MH, cp, ci]
    lib.beom_multi_stats.argtypes = [MH, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    lib.beom_multi_create_ex.argtypes = [C.POINTER(BeomParams), ci, C.POINTER(ci), ci, ipp, ipp] + [dpp] * 14 + [C.POINTER(MH), cp, ci]
    lib.beom_multi_download_outputs.argtypes = [MH, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, dpp, C.POINTER(ci), cp, ci]
    lib.beom_multi_download_diag.argtypes = [MH, C.c_void_p, C.c_void_p, C.c_void_p, cp, ci]
    lib.beom_multi_describe.argtypes = [MH] + [C.POINTER(ci)] * 5
    lib.beom_multi_set_option.argtypes = [MH, cp, ci]
    lib.beom_multi_engine.argtypes = [MH, ci, C.POINTER(H)]
    lib.beom_multi_profile_start.argtypes = [MH]
    lib.beom_multi_profile_stop.argtypes = [MH, dpp, C.POINTER(ci), cp, ci]
    lib.beom_rccl_unique_id.argtypes = [C.c_void_p, cp, ci]
    lib.beom_rccl_version.argtypes = [cp, ci]
    lib.beom_multi_window.argtypes = [C.POINTER(BeomParams), ci, ci, ci] + [C.POINTER(ci)] * 4
    lib.beom_multi_create_local.argtypes = [C.POINTER(BeomParams), ci, ci, ci, ci, ci, C.c_void_p,
                                            C.POINTER(BeomStatics), C.POINTER(BeomStatics), C.POINTER(MH), cp, ci]
    lib.beom_multi_create_local_ex.argtypes = [C.POINTER(BeomParams), ci, ci, ci, ci, ci, ci, C.c_void_p,
                                               C.POINTER(BeomStatics), C.POINTER(BeomStatics), C.POINTER(MH), cp, ci]
    lib.beom_multi_set_open_boundaries_local.argtypes = [MH, ci, C.POINTER(ci), ci, C.POINTER(ci), cp, ci]
    lib.beom_multi_upload_local.argtypes = [MH, C.POINTER(BeomState), C.POINTER(BeomState), cp, ci]
    lib.beom_multi_download_local.argtypes = [MH, C.POINTER(BeomState), C.POINTER(BeomState), cp, ci]
    if hasattr(lib, "beom_integral_count"):      # (an older build named by BEOM_HIP_LIB for an A/B of the steps has no integrals)
        lib.beom_integral_count.argtypes = [ci]
        lib.beom_integral_rows.argtypes = [H, ci, ci, dpp, cp, ci]
        lib.beom_integral_combine.argtypes = [dpp, ci, ci, dpp]
        lib.beom_integrals.argtypes = [H, dpp, cp, ci]
        lib.beom_multi_integrals.argtypes = [MH, dpp, cp, ci]
        lib.beom_multi_integral_rows_local.argtypes = [MH, C.POINTER(ci), C.POINTER(ci), dpp, cp, ci]
        for name in ("beom_integral_count", "beom_integral_rows", "beom_integral_combine", "beom_integrals",
                     "beom_multi_integrals", "beom_multi_integral_rows_local"):
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_tracers"):         # (likewise: an older build has no tracers)
        lib.beom_set_tracers.argtypes = [H, ci, cp, ci]
        lib.beom_upload_tracers.argtypes = [H, dpp, dpp, dpp, cp, ci]
        lib.beom_download_tracers.argtypes = [H, dpp, dpp, cp, ci]
        lib.beom_update_tracers.argtypes = [H, cd, cd, cd]
        lib.beom_multi_set_tracers.argtypes = [MH, ci, cp, ci]
        lib.beom_multi_upload_tracers.argtypes = [MH, dpp, dpp, dpp, cp, ci]
        lib.beom_multi_download_tracers.argtypes = [MH, dpp, dpp, cp, ci]
        for name in ("beom_set_tracers", "beom_upload_tracers", "beom_download_tracers", "beom_update_tracers",
                     "beom_multi_set_tracers", "beom_multi_upload_tracers", "beom_multi_download_tracers"):
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_tracer_scheme"):   # (likewise: an older build has one tracer scheme)
        lib.beom_set_tracer_scheme.argtypes = [H, ci, cp, ci]
        lib.beom_multi_set_tracer_scheme.argtypes = [MH, ci, cp, ci]
        lib.beom_set_tracer_scheme.restype = ci
        lib.beom_multi_set_tracer_scheme.restype = ci
    if hasattr(lib, "beom_set_tracer_mixing"):   # (likewise: an older build has no tracer mixing)
        lib.beom_set_tracer_mixing.argtypes = [H, dpp, dpp, dpp, cp, ci]
        lib.beom_multi_set_tracer_mixing.argtypes = [MH, dpp, dpp, dpp, cp, ci]
        lib.beom_update_tracer_mixing.argtypes = [H]
        for name in TRACER_MIX_EXPORTS:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_tracer_vmixing"):  # (likewise: an older build has no vertical tracer mixing)
        lib.beom_set_tracer_vmixing.argtypes = [H, dpp, cp, ci]
        lib.beom_multi_set_tracer_vmixing.argtypes = [MH, dpp, cp, ci]
        lib.beom_update_tracer_vmixing.argtypes = [H]
        for name in TRACER_VMIX_EXPORTS:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_floats"):          # (likewise: an older build has no floats)
        lib.beom_set_floats.argtypes = [H, C.c_int64, ci, ci, cp, ci]
        lib.beom_upload_floats.argtypes = [H, dpp, dpp, ipp, cp, ci]
        lib.beom_download_floats.argtypes = [H, dpp, dpp, ipp, ipp, cp, ci]
        lib.beom_download_float_track.argtypes = [H, dpp, C.POINTER(ci), C.POINTER(ci), cp, ci]
        lib.beom_update_floats.argtypes = [H, ci]
        for name in ("beom_set_floats", "beom_upload_floats", "beom_download_floats", "beom_download_float_track",
                     "beom_update_floats"):
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_multi_set_floats"):    # (likewise: an older build has no floats on bands)
        ullp = C.POINTER(C.c_ulonglong)
        vpp = C.POINTER(C.c_void_p)
        lib.beom_multi_set_floats.argtypes = [MH, C.c_int64, ci, cp, ci]
        lib.beom_multi_upload_floats.argtypes = [MH, dpp, dpp, ipp, cp, ci]
        lib.beom_multi_download_floats.argtypes = [MH, dpp, dpp, ipp, ipp, cp, ci]
        lib.beom_multi_update_floats.argtypes = [MH, ci]
        lib.beom_band_floats_set.argtypes = [H, C.c_int64, ci, ci, ci, ci, ci, ci, ci, ci, ci, cp, ci]
        lib.beom_band_floats_check.argtypes = [H, dpp, dpp, ullp, cp, ci]
        lib.beom_band_floats_commit.argtypes = [H, ipp, cp, ci]
        lib.beom_band_floats_launch.argtypes = [H, ci]
        lib.beom_band_floats_ingest.argtypes = [H]
        lib.beom_band_floats_boxes.argtypes = [H, vpp, vpp, vpp, vpp, C.POINTER(C.c_size_t)]
        lib.beom_band_floats_download.argtypes = [H, dpp, dpp, ipp, ipp, ullp, cp, ci]
        for name in MULTI_FLOAT_EXPORTS:
            getattr(lib, name).restype = ci
    for stem, names in (("moments", MOMENT_EXPORTS), ("tracer_moments", TRACER_MOMENT_EXPORTS)):
        if not hasattr(lib, "beom_set_" + stem):     # (likewise: an older build has no moments, or no tracer moments)
            continue
        ip, llp = C.POINTER(ci), C.POINTER(C.c_longlong)
        for pre, T, err in (("beom_", H, []), ("beom_multi_", MH, [cp, ci])):
            getattr(lib, pre + "set_" + stem).argtypes = [T, ci, ci, cp, ci]
            getattr(lib, pre + "reset_" + stem).argtypes = [T] + err
            getattr(lib, pre + "download_" + stem).argtypes = [T, dpp, dpp, dpp, llp, ip, ip, cp, ci]
        getattr(lib, "beom_sample_" + stem).argtypes = [H]
        for name in names:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_harmonics"):       # (likewise: an older build has no harmonics)
        ip, llp = C.POINTER(ci), C.POINTER(C.c_longlong)
        lib.beom_harmonic_weights.argtypes = [cd, cd, dpp, dpp]
        lib.beom_sample_harmonics.argtypes = [H, cd]
        for pre, T, err in (("beom_", H, []), ("beom_multi_", MH, [cp, ci])):
            getattr(lib, pre + "set_harmonics").argtypes = [T, ci, dpp, ci, ci, cp, ci]
            getattr(lib, pre + "reset_harmonics").argtypes = [T] + err
            getattr(lib, pre + "download_harmonics").argtypes = [T, dpp, dpp, dpp, dpp, llp, ip, ip, cp, ci]
        for name in HARMONIC_EXPORTS:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_forcing"):         # (likewise: an older build has no forcing in time)
        ip = C.POINTER(ci)
        lib.beom_forcing_weight.argtypes = [ci, dpp, cd, cd, ip, ip, dpp]
        lib.beom_apply_forcing.argtypes = [H, cd, cp, ci]
        for pre, T in (("beom_", H), ("beom_multi_", MH)):
            getattr(lib, pre + "set_forcing").argtypes = [T, ci, ci, dpp, cd, dpp, cp, ci]
            getattr(lib, pre + "download_forcing").argtypes = [T, dpp, dpp, cp, ci]
        for name in FORCING_EXPORTS:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_series"):          # (likewise: an older build has no series)
        ip = C.POINTER(ci)
        lib.beom_series_count.argtypes = [ci, ci]
        lib.beom_set_series.argtypes = [H, ci, ci, ci, cp, ci]
        lib.beom_band_set_series.argtypes = [H, ci, ci, ci, ci, ci, cp, ci]
        lib.beom_sample_series.argtypes = [H]
        lib.beom_download_series.argtypes = [H, dpp, ip, ip, cp, ci]
        lib.beom_multi_set_series.argtypes = [MH, ci, ci, ci, cp, ci]
        lib.beom_multi_download_series.argtypes = [MH, dpp, ip, ip, cp, ci]
        for name in SERIES_EXPORTS:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_column_series"):   # (likewise: an older build has no column series)
        ip = C.POINTER(ci)
        lib.beom_set_column_series.argtypes = [H, ci, ci, ci, ci, ci, cp, ci]
        lib.beom_sample_column_series.argtypes = [H]
        lib.beom_download_column_series.argtypes = [H, dpp, ip, ip, cp, ci]
        lib.beom_multi_set_column_series.argtypes = [MH, ci, ci, ci, ci, ci, cp, ci]
        lib.beom_multi_download_column_series.argtypes = [MH, dpp, ip, ip, cp, ci]
        for name in COLUMN_SERIES_EXPORTS:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_tracer_column_series"):   # (likewise: an older build has no tracer column series)
        ip = C.POINTER(ci)
        lib.beom_set_tracer_column_series.argtypes = [H, ci, ci, ci, ci, ci, cp, ci]
        lib.beom_sample_tracer_column_series.argtypes = [H]
        lib.beom_download_tracer_column_series.argtypes = [H, dpp, ip, ip, cp, ci]
        lib.beom_multi_set_tracer_column_series.argtypes = [MH, ci, ci, ci, ci, ci, cp, ci]
        lib.beom_multi_download_tracer_column_series.argtypes = [MH, dpp, ip, ip, cp, ci]
        for name in TRACER_COLUMN_SERIES_EXPORTS:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_maps"):            # (likewise: an older build has no maps)
        ip = C.POINTER(ci)
        lib.beom_maps_count.argtypes = [ci, ci, ci]
        lib.beom_set_maps.argtypes = [H, ci, ci, ci, ci, cp, ci]
        lib.beom_sample_maps.argtypes = [H]
        lib.beom_download_maps.argtypes = [H, dpp, ip, ip, cp, ci]
        lib.beom_multi_set_maps.argtypes = [MH, ci, ci, ci, ci, cp, ci]
        lib.beom_multi_download_maps.argtypes = [MH, dpp, ip, ip, cp, ci]
        for name in MAPS_EXPORTS:
            getattr(lib, name).restype = ci
    if hasattr(lib, "beom_set_tracer_series"):   # (likewise: an older build has no tracer series)
        ip = C.POINTER(ci)
        lib.beom_tracer_series_count.argtypes = [ci, ci, ci]
        lib.beom_set_tracer_series.argtypes = [H, ci, ci, ci, cp, ci]
        lib.beom_band_set_tracer_series.argtypes = [H, ci, ci, ci, ci, ci, cp, ci]
        lib.beom_sample_tracer_series.argtypes = [H]
        lib.beom_download_tracer_series.argtypes = [H, dpp, ip, ip, cp, ci]
        lib.beom_multi_set_tracer_series.argtypes = [MH, ci, ci, ci, cp, ci]
        lib.beom_multi_download_tracer_series.argtypes = [MH, dpp, ip, ip, cp, ci]
        for name in TRACER_SERIES_EXPORTS:
            getattr(lib, name).restype = ci
    for name in ("beom_multi_create", "beom_multi_destroy", "beom_multi_count", "beom_multi_band",
                 "beom_multi_upload_state", "beom_multi_download_state", "beom_multi_step", "beom_multi_sync",
                 "beom_multi_stats", "beom_multi_create_ex", "beom_multi_describe", "beom_multi_engine",
                 "beom_multi_download_outputs", "beom_multi_download_diag", "beom_multi_set_open_boundaries",
                 "beom_multi_set_option", "beom_multi_profile_start", "beom_multi_profile_stop", "beom_rccl_unique_id", "beom_rccl_version",
                 "beom_multi_window", "beom_multi_create_local", "beom_multi_create_local_ex", "beom_multi_set_open_boundaries_local",
                 "beom_multi_upload_local", "beom_multi_download_local"):
        getattr(lib, name).restype = ci
    for name in ("beom_device_count", "beom_create", "beom_destroy", "beom_upload_state",
                 "beom_download_state", "beom_download_scratch", "beom_step", "beom_sync",
                 "beom_update_h", "beom_update_mont_rvor_pvor_dive_kine", "beom_update_viscosity",
                 "beom_update_u", "beom_update_v", "beom_rebuild_fluxes", "beom_distribute_stress",
                 "beom_device_field", "beom_is_dense", "beom_profile_steps", "beom_set_stream",
                 "beom_profile_start", "beom_profile_stop", "beom_set_option", "beom_step_phase",
                 "beom_pack_rows", "beom_unpack_rows", "beom_pack_rows2", "beom_unpack_rows2", "beom_download_outputs", "beom_set_open_boundaries"):
        getattr(lib, name).restype = ci
    if lib.beom_abi_version() != BEOM_ABI_VERSION:
        raise RuntimeError("ABI mismatch")
    _lib = lib
    return lib


MULTI_FLOAT_EXPORTS = ("beom_multi_set_floats", "beom_multi_upload_floats", "beom_multi_download_floats", "beom_multi_update_floats",
                       "beom_band_floats_set", "beom_band_floats_check", "beom_band_floats_commit", "beom_band_floats_launch",
                       "beom_band_floats_ingest", "beom_band_floats_boxes", "beom_band_floats_download")
MOMENT_EXPORTS = ("beom_set_moments", "beom_reset_moments", "beom_sample_moments", "beom_download_moments",
                  "beom_multi_set_moments", "beom_multi_reset_moments", "beom_multi_download_moments")
TRACER_MOMENT_EXPORTS = ("beom_set_tracer_moments", "beom_reset_tracer_moments", "beom_sample_tracer_moments",
                         "beom_download_tracer_moments", "beom_multi_set_tracer_moments", "beom_multi_reset_tracer_moments",
                         "beom_multi_download_tracer_moments")
HARMONIC_EXPORTS = ("beom_harmonic_weights", "beom_set_harmonics", "beom_reset_harmonics", "beom_sample_harmonics",
                    "beom_download_harmonics", "beom_multi_set_harmonics", "beom_multi_reset_harmonics",
                    "beom_multi_download_harmonics")
TRACER_MIX_EXPORTS = ("beom_set_tracer_mixing", "beom_update_tracer_mixing", "beom_multi_set_tracer_mixing")
TRACER_VMIX_EXPORTS = ("beom_set_tracer_vmixing", "beom_update_tracer_vmixing", "beom_multi_set_tracer_vmixing")
SERIES_EXPORTS = ("beom_series_count", "beom_set_series", "beom_sample_series", "beom_download_series", "beom_band_set_series",
                  "beom_multi_set_series", "beom_multi_download_series")
TRACER_SERIES_EXPORTS = ("beom_tracer_series_count", "beom_set_tracer_series", "beom_sample_tracer_series",
                         "beom_download_tracer_series", "beom_band_set_tracer_series", "beom_multi_set_tracer_series",
                         "beom_multi_download_tracer_series")
COLUMN_SERIES_EXPORTS = ("beom_set_column_series", "beom_sample_column_series", "beom_download_column_series",
                         "beom_multi_set_column_series", "beom_multi_download_column_series")
TRACER_COLUMN_SERIES_EXPORTS = ("beom_set_tracer_column_series", "beom_sample_tracer_column_series",
                                "beom_download_tracer_column_series", "beom_multi_set_tracer_column_series",
                                "beom_multi_download_tracer_column_series")
MAPS_EXPORTS = ("beom_maps_count", "beom_set_maps", "beom_sample_maps", "beom_download_maps", "beom_multi_set_maps",
                "beom_multi_download_maps")
FORCING_EXPORTS = ("beom_forcing_weight", "beom_set_forcing", "beom_apply_forcing", "beom_download_forcing",
                   "beom_multi_set_forcing", "beom_multi_download_forcing")
ERR_FLOAT_REACH, ERR_FLOAT_OVERFLOW, ERR_FLOAT_CLAIM = -41, -42, -43      # beom_multi_download_floats (include/beom_hip.h)

EXPORTS = ("beom_abi_version", "beom_device_count", "beom_device_pci_bus_id", "beom_info", "beom_download_diag", "beom_create", "beom_destroy", "beom_set_rigid_lid", "beom_download_pressure",
           "beom_upload_state", "beom_download_state", "beom_download_scratch", "beom_step",
           "beom_sync", "beom_update_h", "beom_update_mont_rvor_pvor_dive_kine",
           "beom_update_viscosity", "beom_update_u", "beom_update_v", "beom_rebuild_fluxes",
           "beom_distribute_stress", "beom_device_field", "beom_is_dense", "beom_profile_steps",
           "beom_set_stream", "beom_profile_start", "beom_profile_stop", "beom_set_option",
           "beom_step_phase", "beom_pack_rows", "beom_unpack_rows", "beom_pack_rows2", "beom_unpack_rows2", "beom_download_outputs",
           "beom_set_open_boundaries",
           "beom_multi_create", "beom_multi_destroy", "beom_multi_count", "beom_multi_band",
           "beom_multi_upload_state", "beom_multi_download_state", "beom_multi_step", "beom_multi_sync",
           "beom_multi_stats", "beom_multi_create_ex", "beom_multi_describe", "beom_multi_engine",
           "beom_multi_download_outputs", "beom_multi_download_diag", "beom_multi_set_open_boundaries",
           "beom_multi_set_option", "beom_multi_profile_start", "beom_multi_profile_stop", "beom_rccl_unique_id", "beom_rccl_version",
           "beom_multi_window", "beom_multi_create_local", "beom_multi_create_local_ex", "beom_multi_set_open_boundaries_local",
           "beom_multi_upload_local", "beom_multi_download_local",
           "beom_integral_count", "beom_integral_rows", "beom_integral_combine", "beom_integrals",
           "beom_multi_integrals", "beom_multi_integral_rows_local",
           "beom_set_tracers", "beom_upload_tracers", "beom_download_tracers", "beom_update_tracers",
           "beom_multi_set_tracers", "beom_multi_upload_tracers", "beom_multi_download_tracers",
           "beom_set_tracer_scheme", "beom_multi_set_tracer_scheme",
           "beom_set_floats", "beom_upload_floats", "beom_download_floats", "beom_download_float_track", "beom_update_floats",
           ) + MOMENT_EXPORTS + MULTI_FLOAT_EXPORTS + TRACER_MOMENT_EXPORTS + SERIES_EXPORTS + TRACER_MIX_EXPORTS + TRACER_VMIX_EXPORTS + TRACER_SERIES_EXPORTS + HARMONIC_EXPORTS + FORCING_EXPORTS + COLUMN_SERIES_EXPORTS + TRACER_COLUMN_SERIES_EXPORTS + MAPS_EXPORTS

STATE_NAMES = ("hlay", "u", "v", "h_u", "h_v", "rs_h", "dmdx", "dmdy", "v_cc", "v_ll",
               "tt3d", "tb3d", "tu3d")
SCRATCH_NAMES = ("mont", "rvor", "pvor", "dive", "d2hx", "d2hy")


class BeomError(RuntimeError):
    pass


INTEGRAL_NAMES = ("vol", "ke", "ens", "circ")


def combine_integral_rows(rows) -> np.ndarray:
    """beom_integral_combine (host only, no device): rows[nrows, count] in global row order -> the count sums, by the
    pairwise tree over rows (rows padded with +0.0 to a power of two)."""
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    if rows.ndim != 2 or rows.shape[0] < 1 or rows.shape[1] < 1:
        raise BeomError("combine_integral_rows: rows[nrows, count] expected, got shape %s" % (rows.shape,))
    out = np.zeros(rows.shape[1])
    rc = load().beom_integral_combine(_dp(rows), rows.shape[0], rows.shape[1], _dp(out))
    if rc != 0:
        raise BeomError("beom_integral_combine %d" % rc)
    return out


def scale_integrals(raw: np.ndarray, prm: BeomParams) -> dict:
    """The raw sums of beom_integrals and the figures they stand for: volume_m3[l] = dl^2 * vol, kinetic_J[l] =
    0.5 * rhon(l) * dl^2 * ke, enstrophy[l] and circulation[l] as the domain sums, potential_J = 0.5 * rhon(1) * grav * dl^2 *
    eta2 (the barotropic part only; with a rigid lid eta is the column misfit)."""
    nl = prm.nlay
    q = np.asarray(raw[:4 * nl]).reshape(nl, 4)
    dl2 = prm.dl * prm.dl
    rhon = np.array(list(prm.rhon)[:nl])
    return {"raw": np.array(raw), "vol": q[:, 0].copy(), "ke": q[:, 1].copy(), "ens": q[:, 2].copy(), "circ": q[:, 3].copy(),
            "eta2": float(raw[4 * nl]),
            "volume_m3": dl2 * q[:, 0], "kinetic_J": 0.5 * rhon * dl2 * q[:, 1], "enstrophy": q[:, 2].copy(),
            "circulation": q[:, 3].copy(), "potential_J": 0.5 * rhon[0] * prm.grav * dl2 * float(raw[4 * nl])}


TRACER_SCHEMES = {"upstream": 1, "limited": 2}


class _Handle:
    """What the mixins below ask of the handle class that joins them: `_prefix`, the prefix of its C symbols ("beom_" on Engine,
    "beom_multi_" on MultiEngine and so on BandEngine); the calls differ only by it."""

    def _fn(self, name):
        return getattr(self.lib, self._prefix + name)

    @property
    def _multi(self) -> bool:
        return self._prefix == "beom_multi_"


class _Tracers(_Handle):
    """Passive tracers of a handle (beom_set_tracers, include/beom_hip.h): shared by Engine and MultiEngine, whose C calls
    differ only by name.  Arrays: q, ctrg [ntrc, nlay, ndeg+1] (the layer CONTENT thickness x concentration, and the
    relaxation concentration), rq [ntrc, nlay, ndeg+1, 2] (the tendency history, as rs_h per tracer)."""

    ntrc = 0

    def set_tracers(self, n: int):
        """Allocates n tracers (q, rq, ctrg = 0); n = 0 frees them.  Between steps only."""
        self._check(self._fn("set_tracers")(self.h, int(n), self._err, ERRLEN))
        self.ntrc = int(n)

    def set_tracer_scheme(self, scheme):
        """1 | "upstream" (the default) or 2 | "limited" (Koren's flux-limited third-order faces, beom_set_tracer_scheme).  Between
        steps only; kept for the handle's life, whatever set_tracers does afterwards."""
        scheme = TRACER_SCHEMES.get(scheme, scheme)
        if isinstance(scheme, str):
            raise BeomError("tracer scheme %r (1 | 'upstream', 2 | 'limited')" % (scheme,))
        self._check(self._fn("set_tracer_scheme")(self.h, int(scheme), self._err, ERRLEN))

    def set_tracer_mixing(self, kappa=None, decay=None, source=None):
        """Lateral diffusion kappa (m2/s), decay (1/s) and source (concentration per second) of the tracers, applied in a
        launch of its own in front of every step's tracer sweep (beom_set_tracer_mixing).  A scalar, [ntrc] or [ntrc, nlay]
        each, broadcast to [ntrc, nlay]; None = +0.  All None or all zero switches the mixing off.  Between steps only,
        after set_tracers."""
        if not hasattr(self.lib, "beom_set_tracer_mixing"):
            raise BeomError("this libbeom_hip.so has no tracer mixing (beom_set_tracer_mixing)")
        want = (self.ntrc, self.p.nlay)
        co = []
        for name, a in (("kappa", kappa), ("decay", decay), ("source", source)):
            if a is not None:
                a = np.asarray(a, dtype=np.float64)
                if a.ndim > 2 or (a.ndim == 1 and a.shape != want[:1]) or (a.ndim == 2 and a.shape != want):
                    raise BeomError("%s of shape %s: a scalar, %s or %s expected" % (name, a.shape, want[:1], want))
                a = np.ascontiguousarray(np.broadcast_to(a[:, None] if a.ndim == 1 else a, want))
            co.append(a)
        self._check(self._fn("set_tracer_mixing")(self.h, _dp(co[0]), _dp(co[1]), _dp(co[2]), self._err, ERRLEN))

    def set_tracer_vertical_mixing(self, kappa_v=None):
        """Vertical (diapycnal) diffusion kappa_v (m2/s) of the tracers through the nlay - 1 interfaces of every water column,
        implicit in the column, in a launch of its own between the lateral mixing and the tracer sweep
        (beom_set_tracer_vmixing).  A scalar, [nlay-1] or [ntrc, nlay-1], broadcast to [ntrc, nlay-1]; there is no cap.  None
        or all zero switches it off.  Between steps only, after set_tracers."""
        if not hasattr(self.lib, "beom_set_tracer_vmixing"):
            raise BeomError("this libbeom_hip.so has no vertical tracer mixing (beom_set_tracer_vmixing)")
        a = kappa_v
        if a is not None:
            want = (self.ntrc, self.p.nlay - 1)
            a = np.asarray(a, dtype=np.float64)
            if a.ndim > 2 or (a.ndim == 1 and a.shape != want[1:]) or (a.ndim == 2 and a.shape != want):
                raise BeomError("kappa_v of shape %s: a scalar, %s or %s expected" % (a.shape, want[1:], want))
            a = np.ascontiguousarray(np.broadcast_to(a, want))
            if a.size == 0:         # (no tracer or one layer: the library refuses in its own words, and reads no value)
                a = np.zeros(1)
        self._check(self._fn("set_tracer_vmixing")(self.h, _dp(a), self._err, ERRLEN))

    def _trc_array(self, a, tail=()):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.float64)
        want = (self.ntrc, self.p.nlay, self.p.ndeg + 1) + tail
        if a.shape != want:
            raise BeomError("tracer array of shape %s, expected %s" % (a.shape, want))
        return a

    def upload_tracers(self, q=None, rq=None, ctrg=None):
        q, rq, ctrg = self._trc_array(q), self._trc_array(rq, (2,)), self._trc_array(ctrg)
        self._check(self._fn("upload_tracers")(self.h, _dp(q), _dp(rq), _dp(ctrg), self._err, ERRLEN))

    def download_tracers(self) -> dict:
        n = (self.ntrc, self.p.nlay, self.p.ndeg + 1)
        out = {"q": np.zeros(n), "rq": np.zeros(n + (2,))}
        self._check(self._fn("download_tracers")(self.h, _dp(out["q"]), _dp(out["rq"]), self._err, ERRLEN))
        return out

    def set_concentration(self, c):
        """Uploads q = c * hlay with the handle's current hlay (multiplied on the host); c broadcasts to [ntrc, nlay, ndeg+1]."""
        h = self.download(("hlay",))["hlay"]
        q = np.ascontiguousarray(np.broadcast_to(np.asarray(c, dtype=np.float64), (self.ntrc,) + h.shape) * h[None])
        self.upload_tracers(q=q)
        return q


class _Floats(_Handle):
    """Lagrangian floats of a handle (beom_set_floats, include/beom_hip.h): positions x, y in grid units (cell (i, j) spans
    [i-1, i] x [j-1, j]), a fixed 1-based layer per float, moved by every step with Heun's method on the layer velocities.
    Shared by Engine and MultiEngine (floats on bands: replicated slots and hand-over records, no track recorder)."""

    nfloats = 0
    float_records = 0

    def set_floats(self, x, y, layer, records: int = 0, stride: int = 1, capacity: int = 0):
        """Replaces the handle's floats by these (arrays of one length; an empty x frees them) and zeroes their `rejected`
        counters.  records > 0: a recorder of that many records (x, y, h) per float, one behind every step with
        tstp % stride == 0 (download_float_track); single handles only.  capacity (MultiEngine): records an outbox holds per
        side and step, 0 = max(4096, n / 8).  Between steps only."""
        x = np.ascontiguousarray(x, dtype=np.float64).ravel()
        y = np.ascontiguousarray(y, dtype=np.float64).ravel()
        layer = np.ascontiguousarray(np.broadcast_to(np.asarray(layer, dtype=np.int32), x.shape), dtype=np.int32)
        if y.shape != x.shape:
            raise BeomError("set_floats: x of %d positions, y of %d" % (x.size, y.size))
        if self._multi:
            if records > 0:
                raise BeomError("beom_hip error -6: set_floats: bands keep no track recorder (records = %d): a float's records would be "
                                "spread over the bands it has visited; record on a single handle" % records)
            free = lambda: self.lib.beom_multi_set_floats(self.h, 0, 0, None, 0)
            self._check(self.lib.beom_multi_set_floats(self.h, x.size, int(capacity), self._err, ERRLEN))
            upload = self.lib.beom_multi_upload_floats
        else:
            free = lambda: self.lib.beom_set_floats(self.h, 0, 0, 1, None, 0)
            self._check(self.lib.beom_set_floats(self.h, x.size, int(records), int(stride), self._err, ERRLEN))
            upload = self.lib.beom_upload_floats
        self.nfloats, self.float_records = 0, 0
        if x.size:
            try:
                self._check(upload(self.h, _dp(x), _dp(y), _ip(layer), self._err, ERRLEN))
            except BeomError:
                free()                                                   # (refused positions: the handle carries no floats)
                raise
            self.nfloats, self.float_records = int(x.size), int(records)

    def download_floats(self) -> dict:
        n = self.nfloats
        out = {"x": np.zeros(n), "y": np.zeros(n), "layer": np.zeros(n, dtype=np.int32), "rejected": np.zeros(n, dtype=np.int32)}
        self._check(self._fn("download_floats")(self.h, _dp(out["x"]), _dp(out["y"]), _ip(out["layer"]), _ip(out["rejected"]), self._err, ERRLEN))
        return out

    def download_float_track(self) -> dict:
        """The records held, oldest first, and empties the recorder: x, y, h [count, nfloats], tstp [count]."""
        rec = np.zeros((max(self.float_records, 1), 3, self.nfloats))
        tstp = (C.c_int * max(self.float_records, 1))()
        count = C.c_int(0)
        self._check(self.lib.beom_download_float_track(self.h, _dp(rec), C.byref(count), tstp, self._err, ERRLEN))
        k = count.value
        return {"x": rec[:k, 0].copy(), "y": rec[:k, 1].copy(), "h": rec[:k, 2].copy(), "tstp": np.array(list(tstp)[:k], dtype=np.int64)}

    def update_floats(self, stage: int):
        """Per-sweep entry: stage 1 or stage 2 of the scheme on the velocities as they stand (no record)."""
        rc = self._fn("update_floats")(self.h, int(stage))
        if rc != 0:
            raise BeomError("beom_update_floats(stage %d) = %d (floats set and uploaded? stage 1 or 2?)" % (stage, rc))


class _Accum(_Handle):
    """What _Moments and _TracerMoments share: set, reset and download of a device-side time accumulator through the exports
    beom_[multi_]{set,reset,download}_<stem>, the level asked of the handle (info(<stem>))."""

    def _accum_fn(self, op, stem):
        return self._fn("%s_%s" % (op, stem))

    def _accum_set(self, stem, level, stride):
        self._check(self._accum_fn("set", stem)(self.h, int(level), int(stride), self._err, ERRLEN))

    def _accum_plain(self, op, stem, what):
        """reset or sample on a single handle: no message comes back, only a code."""
        rc = getattr(self.lib, "beom_%s_%s" % (op, stem))(self.h)
        if rc != 0:
            raise BeomError("beom_hip error %d: beom_%s_%s (%s set?)" % (rc, op, stem, what))

    def _accum_reset(self, stem, what):
        if self._multi:
            self._check(self._accum_fn("reset", stem)(self.h, self._err, ERRLEN))
        else:
            self._accum_plain("reset", stem, what)

    def _accum_download(self, stem, lv, counts, nsq, shape, var_key, var):
        """ref, sum [counts[lv >= 2], *shape], at level 3 sq [*nsq, *shape] (nsq a tuple) and out[var_key] = var(sq/n, sum/n)."""
        nq = counts[lv >= 2]
        ref, sm = np.zeros((nq,) + shape), np.zeros((nq,) + shape)
        sq = np.zeros(nsq + shape) if lv >= 3 else None
        count, t0, t1 = C.c_longlong(0), C.c_int(0), C.c_int(0)
        self._check(self._accum_fn("download", stem)(self.h, _dp(ref), _dp(sm), _dp(sq), C.byref(count), C.byref(t0),
                                                     C.byref(t1), self._err, ERRLEN))
        out = {"count": int(count.value), "tstp_first": int(t0.value), "tstp_last": int(t1.value), "ref": ref, "sum": sm}
        n = float(max(out["count"], 1))
        out["mean"] = ref + sm / n
        if sq is not None:
            out["sq"] = sq
            out[var_key] = var(sq / n, sm / n)
        return out


MOMENT_FIELDS = ("hlay", "u", "v", "h_u", "h_v")
MOMENT_PAIRS = ((0, 0), (1, 1), (2, 2), (1, 3), (2, 4))      # the five second moments: (h,h) (u,u) (v,v) (u,h_u) (v,h_v)


class _Moments(_Accum):
    """Time means and second moments of the layer fields (beom_set_moments, include/beom_hip.h): sums shifted by the first
    sample, kept on the device and fed behind every step with tstp % stride == 0.  Shared by Engine and MultiEngine."""

    moment_level = 0

    def set_moments(self, level: int, stride: int = 1):
        """level 1: ref, sum of hlay, u, v; 2: and of h_u, h_v; 3: and the five second moments; 0 frees.  Between steps only."""
        self._accum_set("moments", level, stride)
        self.moment_level = int(level)

    def reset_moments(self):
        """count = 0: the next sample is a first sample (no memory moves)."""
        self._accum_reset("moments", "moments")

    def download_moments(self) -> dict:
        """count, tstp_first, tstp_last; the raw ref, sum [fields, nlay, ndeg+1] and, at level 3, sq [5, nlay, ndeg+1]; the
        derived mean = ref + sum/count and, at level 3, var = sq/count - (sum_a/count)*(sum_b/count) (var[0..2] the variances
        of hlay, u, v; var[3..4] the covariances of (u, h_u), (v, h_v))."""
        self.moment_level = self.info("moments")
        return self._accum_download("moments", self.moment_level, (3, 5), (5,), (self.p.nlay, self.p.ndeg + 1), "var",
                                    lambda q, m: np.stack([q[k] - m[a] * m[b] for k, (a, b) in enumerate(MOMENT_PAIRS)]))


BEOM_MAX_HARMONICS = 4


def harmonic_weights(omega: float, ctim: float):
    """beom_harmonic_weights (host only, no device): (cos, sin) of the FP64 product omega*ctim, the weights of a sample."""
    cw, sw = C.c_double(0.0), C.c_double(0.0)
    rc = load().beom_harmonic_weights(float(omega), float(ctim), C.byref(cw), C.byref(sw))
    if rc != 0:
        raise BeomError("beom_harmonic_weights = %d" % rc)
    return cw.value, sw.value


def derive_harmonics(out: dict) -> dict:
    """Adds the derived keys to a download's raw ref [F, nlay, n], sum [F, 1+2K, nlay, n], gram [1+2K, 1+2K] and count when
    the fit is determined (count >= 1 + 2K and numpy.linalg.solve succeeds); otherwise leaves them absent.  Per element
    G a = (S0, C_1, S_1, ...): mean = ref + a_0, amp_k = hypot(a_{2k-1}, a_{2k}), phase_k = atan2(a_{2k}, a_{2k-1}), all
    [F, K, nlay, n] (mean [F, nlay, n]); eta_amp, eta_phase [K, nlay, n] are those of the interface elevations, by linearity
    the bottom-up cumulative sum over the layers of the hlay coefficients (interface ilay lies on top of layer ilay)."""
    sm, gram = out["sum"], out["gram"]
    nw = gram.shape[0]
    if out["count"] < nw:
        return out
    try:
        a = np.linalg.solve(gram, sm.transpose(1, 0, 2, 3).reshape(nw, -1)).reshape((nw,) + sm.shape[:1] + sm.shape[2:])
    except np.linalg.LinAlgError:
        return out
    if not np.all(np.isfinite(a)):
        return out
    out["mean"] = out["ref"] + a[0]
    out["amp"] = np.stack([np.hypot(a[1 + 2 * k], a[2 + 2 * k]) for k in range(nw // 2)], axis=1)
    out["phase"] = np.stack([np.arctan2(a[2 + 2 * k], a[1 + 2 * k]) for k in range(nw // 2)], axis=1)
    e = np.cumsum(a[1:, 0, ::-1], axis=1)[:, ::-1]            # [2K, nlay, n]: the hlay coefficients summed from the bottom up
    out["eta_amp"] = np.stack([np.hypot(e[2 * k], e[1 + 2 * k]) for k in range(nw // 2)])
    out["eta_phase"] = np.stack([np.arctan2(e[1 + 2 * k], e[2 * k]) for k in range(nw // 2)])
    return out


class _Harmonics(_Handle):
    """Least-squares harmonic analysis of the layer fields (beom_set_harmonics, include/beom_hip.h): per field a reference
    and 1 + 2K sums shifted by it, kept on the device and fed behind every step with tstp % stride == 0; the normal matrix
    on the host.  Shared by Engine and MultiEngine."""

    def _harm_fn(self, op):
        return self._fn(op + "_harmonics")

    def set_harmonics(self, omega=None, level: int = 1, stride: int = 1):
        """omega: up to BEOM_MAX_HARMONICS frequencies in rad/day (None: the handle's tidal frequency w_ti; an empty
        sequence frees); level 1: hlay, u, v; 2: and h_u, h_v.  Between steps only."""
        if omega is None:
            if float(self.prm.w_ti) == 0.0:
                raise BeomError("set_harmonics: the handle has no tide (w_ti = 0): give omega")
            omega = (float(self.prm.w_ti),)
        om = np.ascontiguousarray(np.atleast_1d(omega), dtype=np.float64)
        self._check(self._harm_fn("set")(self.h, int(om.size), _dp(om), int(level), int(stride), self._err, ERRLEN))

    def reset_harmonics(self):
        """count = 0 and a zero normal matrix: the next sample is a first sample (no device memory moves)."""
        if self._multi:
            self._check(self._harm_fn("reset")(self.h, self._err, ERRLEN))
        else:
            rc = self.lib.beom_reset_harmonics(self.h)
            if rc != 0:
                raise BeomError("beom_hip error %d: beom_reset_harmonics (harmonics set?)" % rc)

    def download_harmonics(self) -> dict:
        """count, tstp_first, tstp_last, omega [K]; the raw ref [F, nlay, ndeg+1], sum [F, 1+2K, nlay, ndeg+1] (S0, C_1, S_1,
        ...) and gram [1+2K, 1+2K]; and, when the fit is determined, the keys of derive_harmonics."""
        fn = self._harm_fn("download")
        count, t0, t1 = C.c_longlong(0), C.c_int(0), C.c_int(0)
        om = np.zeros(BEOM_MAX_HARMONICS)
        gram = np.zeros((1 + 2 * BEOM_MAX_HARMONICS) ** 2)
        self._check(fn(self.h, None, None, _dp(gram), _dp(om), C.byref(count), C.byref(t0), C.byref(t1), self._err, ERRLEN))
        k, nf = self.info("harmonics"), 5 if self.info("harmonic_level") >= 2 else 3      # (bands: what band 0 keeps)
        nw, shape = 1 + 2 * k, (self.p.nlay, self.p.ndeg + 1)
        ref, sm = np.zeros((nf,) + shape), np.zeros((nf, nw) + shape)
        self._check(fn(self.h, _dp(ref), _dp(sm), None, None, None, None, None, self._err, ERRLEN))
        out = {"count": int(count.value), "tstp_first": int(t0.value), "tstp_last": int(t1.value), "omega": om[:k].copy(),
               "ref": ref, "sum": sm, "gram": gram[:nw * nw].reshape(nw, nw).copy()}
        return derive_harmonics(out)


FORCING_FIELDS = {"taus": 1, "hdot": 2}      # BEOM_FORCING_TAUS, BEOM_FORCING_HDOT


def forcing_weight(times, period: float, ctim: float):
    """beom_forcing_weight (host only, no device): the frames (k0, k1) and the weight a of time ctim for a frame set with
    these times (days) and period (0 = none)."""
    t = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float64)
    k0, k1, a = C.c_int(0), C.c_int(0), C.c_double(0.0)
    rc = load().beom_forcing_weight(int(t.size), _dp(t), float(period), float(ctim), C.byref(k0), C.byref(k1), C.byref(a))
    if rc != 0:
        raise BeomError("beom_forcing_weight = %d" % rc)
    return k0.value, k1.value, a.value


class _Forcing(_Handle):
    """Forcing in time (beom_set_forcing, include/beom_hip.h): frames of taus [nfr, 2, ndeg+1] or hdot [nfr, nlay, ndeg+1]
    at times in days, interpolated on the device at the top of every step.  Shared by Engine and MultiEngine."""

    def _forcing_shape(self, field):
        if field not in FORCING_FIELDS:
            raise BeomError("forcing field %r: one of %s" % (field, sorted(FORCING_FIELDS)))
        return (2 if field == "taus" else self.p.nlay, self.p.ndeg + 1)

    def set_forcing(self, field: str, times, frames=None, period: float = 0.0):
        """times=None clears the set: the handle reads the arrays it was created with again.  Between steps only."""
        shape = self._forcing_shape(field)
        fn = self._fn("set_forcing")
        if times is None:
            self._check(fn(self.h, FORCING_FIELDS[field], 0, None, 0.0, None, self._err, ERRLEN))
            return
        t = np.ascontiguousarray(np.atleast_1d(times), dtype=np.float64)
        fr = np.ascontiguousarray(frames, dtype=np.float64)
        if fr.shape != (t.size,) + shape:
            raise BeomError("set_forcing(%s): frames %s, expected %s" % (field, fr.shape, (t.size,) + shape))
        self._check(fn(self.h, FORCING_FIELDS[field], int(t.size), _dp(t), float(period), _dp(fr), self._err, ERRLEN))

    def apply_forcing(self, ctim: float):
        """The launches of time ctim alone, as a step would place them (single handles)."""
        if self._multi:
            raise BeomError("apply_forcing: a single handle's call (the bands apply their frames inside their steps)")
        self._check(self.lib.beom_apply_forcing(self.h, float(ctim), self._err, ERRLEN))

    def download_forcing(self) -> dict:
        """{"taus", "hdot"}: what the next sweep would read, in the caller's storage."""
        out = {"taus": np.zeros((2, self.p.ndeg + 1)), "hdot": np.zeros((self.p.nlay, self.p.ndeg + 1))}
        self._check(self._fn("download_forcing")(self.h, _dp(out["taus"]), _dp(out["hdot"]), self._err, ERRLEN))
        return out


TRACER_MOMENT_QUANTITIES = ("q", "c", "fu", "fv")     # content, concentration, upstream face fluxes through the W and S faces


class _TracerMoments(_Accum):
    """Time means of the tracers' content, concentration and upstream face fluxes, and the concentration's second moment
    (beom_set_tracer_moments, include/beom_hip.h): sums shifted by the first sample, kept on the device and fed behind every
    step with tstp % stride == 0, with a level, stride and count of their own.  Shared by Engine and MultiEngine."""

    tracer_moment_level = 0

    def set_tracer_moments(self, level: int, stride: int = 1):
        """level 1: ref, sum of q and c; 2: and of fu, fv; 3: and the second moment of c; 0 frees.  Between steps only, after
        set_tracers."""
        self._accum_set("tracer_moments", level, stride)
        self.tracer_moment_level = int(level)

    def reset_tracer_moments(self):
        """count = 0: the next sample is a first sample (no memory moves)."""
        self._accum_reset("tracer_moments", "tracer moments")

    def download_tracer_moments(self) -> dict:
        """count, tstp_first, tstp_last; the raw ref, sum [quantities, ntrc, nlay, ndeg+1] (TRACER_MOMENT_QUANTITIES; two of them
        at level 1) and, at level 3, sq [ntrc, nlay, ndeg+1]; the derived mean = ref + sum/count and, at level 3,
        var_c = sq/count - (sum_c/count)**2."""
        self.tracer_moment_level = self.info("tracer_moments")
        return self._accum_download("tracer_moments", self.tracer_moment_level, (2, 4), (), (self.ntrc, self.p.nlay, self.p.ndeg + 1),
                                    "var_c", lambda q, m: q - m[1] * m[1])


class _Recorder(_Handle):
    """What _Series, _TracerSeries, _ColumnSeries and _TracerColumnSeries share: a device-side recorder [records][lines][cnt] set and downloaded through the exports
    beom_[multi_]{set,download}_<stem>, and sampled by hand on a single handle (beom_sample_<stem>)."""

    def _recorder_set(self, stem, level, stride, records, *window):
        """-> the level and the record count to keep (0 records once freed).  window: the column series' jlo, jhi."""
        self._check(self._fn("set_" + stem)(self.h, int(level), int(stride), int(records), *window, self._err, ERRLEN))
        return int(level), (int(records) if level else 0)

    def _recorder_download(self, stem, what, level, records, cnt_of, lines):
        """The records held, oldest first: (n, tstp[n], rows[n, lines, cnt_of(level)]); empties the recorder."""
        fn = self._fn("download_" + stem)
        if level < 1:                                                    # (the library says why)
            self._check(fn(self.h, None, None, None, self._err, ERRLEN))
            raise BeomError("download_%s: the handle keeps no %s (set_%s)" % (stem, what, stem))
        rows = np.zeros((max(records, 1), lines, cnt_of(level)))
        tstp = (C.c_int * max(records, 1))()
        count = C.c_int(0)
        self._check(fn(self.h, _dp(rows), tstp, C.byref(count), self._err, ERRLEN))
        n = count.value
        return n, np.array(list(tstp)[:n], dtype=np.int64), rows[:n].copy()

    def _recorder_sample(self, stem, what):
        rc = getattr(self.lib, "beom_sample_" + stem)(self.h)
        if rc != 0:
            raise BeomError("beom_hip error %d: beom_sample_%s (%s set? recorder full?)" % (rc, stem, what))


class _Series(_Recorder):
    """A record of the row sums per sampled step, kept on the device (beom_set_series, include/beom_hip.h): the quantities of
    integral_rows for every row of the frame and, at level 2, the row sums of the layer transports h_u, h_v, written behind
    every step with tstp % stride == 0 without a host copy.  Shared by Engine and MultiEngine."""

    series_level = 0
    series_records = 0

    def set_series(self, level: int, stride: int = 1, records: int = 64):
        """level 1: vol, ke, ens, circ per layer and eta2 per row; 2: and tu, tv per layer; 0 frees.  `records`: what the
        recorder holds between two download_series (a step call that would overflow it is refused).  Between steps only."""
        self.series_level, self.series_records = self._recorder_set("series", level, stride, records)

    def download_series(self) -> dict:
        """The records held, oldest first, and empties the recorder.  count, tstp[n]; rows[n, M, cnt] (M = mm+1 rows in global
        order); raw[n, 4*nlay+1] = combine_integral_rows per record (scale_integrals gives the figures); the views vol, ke,
        ens, circ [n, M, nlay] and eta2 [n, M]; at level 2 tu, tv [n, M, nlay], the row sums of the stored transports h_u,
        h_v (thickness * velocity through a cell's W resp. S face, m^2/s), and psi[n, M, nlay] = dl * cumsum(tv, layers):
        the volume transport (m^3/s) above the base of layer l through the south faces of row j."""
        nl, M = self.p.nlay, self.p.mm + 1
        n, tstp, rows = self._recorder_download("series", "series", self.series_level, self.series_records,
                                                lambda lv: self.lib.beom_series_count(nl, lv), M)
        q = rows[:, :, :4 * nl].reshape(n, M, nl, 4)
        out = {"count": n, "tstp": tstp, "rows": rows,
               "raw": np.array([combine_integral_rows(r[:, :4 * nl + 1]) for r in rows]).reshape(n, 4 * nl + 1),
               "eta2": rows[:, :, 4 * nl]}
        for k, name in enumerate(INTEGRAL_NAMES):
            out[name] = q[..., k]
        if self.series_level >= 2:
            out["tu"], out["tv"] = rows[:, :, 4 * nl + 1:5 * nl + 1], rows[:, :, 5 * nl + 1:6 * nl + 1]
            out["psi"] = float(self.p.dl) * np.cumsum(out["tv"], axis=2)
        return out


class _ColumnSeries(_Recorder):
    """A record of the sums along columns per sampled step, kept on the device (beom_set_column_series, include/beom_hip.h):
    the series' quantities for every column of the frame — at level 2 the layer transports through a column's W faces —
    with a level, stride, row window and recorder of its own.  Engine keeps one; MultiEngine refuses (a column's tree
    crosses the bands)."""

    column_series_level = 0
    column_series_records = 0

    def set_column_series(self, level: int, stride: int = 1, records: int = 64, rows=None):
        """level 1: vol, ke, ens, circ per layer and eta2 per column; 2: and tu, tv per layer; 0 frees.  `records`: what the
        recorder holds between two download_column_series (a step call that would overflow it is refused).  rows = (jlo,
        jhi): only these rows of a column count (a strait that spans part of it); None = all, 1..mm+1.  Between steps only."""
        jlo, jhi = (1, self.p.mm + 1) if rows is None else rows
        self.column_series_level, self.column_series_records = self._recorder_set("column_series", level, stride, records,
                                                                                  int(jlo), int(jhi))

    def download_column_series(self) -> dict:
        """The records held, oldest first, and empties the recorder.  count, tstp[n]; cols[n, L, cnt] (L = lm+1 columns);
        the views vol, ke, ens, circ [n, L, nlay] and eta2 [n, L]; at level 2 tu, tv [n, L, nlay], the column sums of the
        stored transports h_u, h_v, and phi[n, L, nlay] = dl * cumsum(tu, layers): the volume transport (m^3/s) above the
        base of layer l through the W faces of column i.  total[n, 4*nlay+1] = the integrals' tree over the columns of each
        record: close to integrals()["raw"] but NOT its bits — the integrals add along rows first, this adds along columns
        first (both pairwise trees over the same terms)."""
        nl, L = self.p.nlay, self.p.lm + 1
        n, tstp, cols = self._recorder_download("column_series", "column series", self.column_series_level,
                                                self.column_series_records, lambda lv: self.lib.beom_series_count(nl, lv), L)
        q = cols[:, :, :4 * nl].reshape(n, L, nl, 4)
        out = {"count": n, "tstp": tstp, "cols": cols,
               "total": np.array([combine_integral_rows(c[:, :4 * nl + 1]) for c in cols]).reshape(n, 4 * nl + 1),
               "eta2": cols[:, :, 4 * nl]}
        for k, name in enumerate(INTEGRAL_NAMES):
            out[name] = q[..., k]
        if self.column_series_level >= 2:
            out["tu"], out["tv"] = cols[:, :, 4 * nl + 1:5 * nl + 1], cols[:, :, 5 * nl + 1:6 * nl + 1]
            out["phi"] = float(self.p.dl) * np.cumsum(out["tu"], axis=2)
        return out


TRACER_SERIES_NAMES = ("inv", "var", "fu", "fv", "cmin", "cmax")


class _TracerSeries(_Recorder):
    """A record per sampled step of the tracers' row inventories, variance, face fluxes and bounds, kept on the device
    (beom_set_tracer_series, include/beom_hip.h), with a level, stride and recorder of its own beside the series.  Shared by
    Engine and MultiEngine."""

    tracer_series_level = 0
    tracer_series_records = 0

    def set_tracer_series(self, level: int, stride: int = 1, records: int = 64):
        """level 1: inv, var per tracer and layer; 2: and fu, fv; 3: and cmin, cmax; 0 frees.  `records`: what the recorder
        holds between two download_tracer_series (a step call that would overflow it is refused).  Between steps only, after
        set_tracers."""
        self.tracer_series_level, self.tracer_series_records = self._recorder_set("tracer_series", level, stride, records)

    def download_tracer_series(self) -> dict:
        """The records held, oldest first, and empties the recorder.  count, tstp[n]; rows[n, M, cnt] (M = mm+1 rows in global
        order); the views inv, var (row sums of q and of q*c) and, at level >= 2, fu, fv (row sums of the upstream face fluxes
        through the W resp. S faces) and, at level 3, cmin, cmax (the concentration's bounds over the row's wet cells, +inf,
        -inf where there is none), each [n, M, ntrc, nlay]; total[n, ntrc, nlay] = combine_integral_rows of inv; at level
        >= 2 transport = dl * fv, the tracer transport through the south faces of row j."""
        nl, M = self.p.nlay, self.p.mm + 1
        lv = self.info("tracer_series")                                  # (set_tracers with another count frees it)
        n, tstp, rows = self._recorder_download("tracer_series", "tracer series", lv, self.tracer_series_records,
                                                lambda lv: self.lib.beom_tracer_series_count(self.ntrc, nl, lv), M)
        self.tracer_series_level = lv
        nq = 2 * lv
        q = rows.reshape(n, M, self.ntrc, nl, nq)
        out = {"count": n, "tstp": tstp, "rows": rows}
        for m in range(nq):
            out[TRACER_SERIES_NAMES[m]] = q[..., m]
        out["total"] = np.array([combine_integral_rows(np.ascontiguousarray(r.reshape(M, self.ntrc * nl)))
                                 for r in out["inv"]]).reshape(n, self.ntrc, nl)
        if lv >= 2:
            out["transport"] = float(self.p.dl) * out["fv"]
        return out


class _TracerColumnSeries(_Recorder):
    """A record per sampled step of the tracers' column inventories, variance, face fluxes and bounds, kept on the device
    (beom_set_tracer_column_series, include/beom_hip.h): the tracer series' quantities for every column of the frame, with a
    level, stride, row window and recorder of its own.  Engine keeps one; MultiEngine refuses (a column's tree crosses the
    bands)."""

    tracer_column_series_records = 0

    def set_tracer_column_series(self, level: int, stride: int = 1, records: int = 64, rows=None):
        """level 1: inv, var per tracer and layer; 2: and fu, fv; 3: and cmin, cmax; 0 frees.  `records`: what the recorder
        holds between two download_tracer_column_series (a step call that would overflow it is refused).  rows = (jlo, jhi):
        only these rows of a column count; None = all, 1..mm+1.  Between steps only, after set_tracers."""
        jlo, jhi = (1, self.p.mm + 1) if rows is None else rows
        _, self.tracer_column_series_records = self._recorder_set("tracer_column_series", level, stride, records, int(jlo), int(jhi))

    def download_tracer_column_series(self) -> dict:
        """The records held, oldest first, and empties the recorder.  count, tstp[n]; cols[n, L, cnt] (L = lm+1 columns); the
        views inv, var (column sums of q and of q*c) and, at level >= 2, fu, fv (column sums of the upstream face fluxes
        through the W resp. S faces) and, at level 3, cmin, cmax (the concentration's bounds over the column's wet cells
        inside the row window, +inf, -inf where there is none), each [n, L, ntrc, nlay]; at level >= 2 transport = dl * fu,
        the tracer transport of layer l through the W faces of column i.  total[n, ntrc, nlay] = the integrals' tree over
        the columns of inv: close to download_tracer_series()["total"] but NOT its bits — the tracer series adds along rows
        first, this adds along columns first (both pairwise trees over the same terms)."""
        nl, L = self.p.nlay, self.p.lm + 1
        lv = 0 if self._multi else self.info("tracer_column_series")      # (set_tracers with another count frees it)
        n, tstp, cols = self._recorder_download("tracer_column_series", "tracer column series", lv, self.tracer_column_series_records,
                                                lambda lv: self.lib.beom_tracer_series_count(self.ntrc, nl, lv), L)
        nq = 2 * lv
        q = cols.reshape(n, L, self.ntrc, nl, nq)
        out = {"count": n, "tstp": tstp, "cols": cols}
        for m in range(nq):
            out[TRACER_SERIES_NAMES[m]] = q[..., m]
        out["total"] = np.array([combine_integral_rows(np.ascontiguousarray(c.reshape(L, self.ntrc * nl)))
                                 for c in out["inv"]]).reshape(n, self.ntrc, nl)
        if lv >= 2:
            out["transport"] = float(self.p.dl) * out["fu"]
        return out


class _Maps(_Recorder):
    """A record of sums over aligned B x B blocks of cells per sampled step, kept on the device (beom_set_maps,
    include/beom_hip.h): coarse maps of thickness, velocity, kinetic energy, transports and tracer content in time, with a
    level, block edge, stride and recorder of their own.  Engine keeps them; MultiEngine refuses (a block's tree must not
    cross a seam between bands)."""

    maps_records = 0

    def set_maps(self, level: int, block: int = 8, stride: int = 1, records: int = 16):
        """level 1: n per block and h, u, v per layer; 2: and ke, hu, hv; 3: and the content q per tracer and layer (after
        set_tracers); 0 frees.  block: the edge B of a block, a power of two in 2..64.  `records`: what the recorder holds
        between two download_maps (a step call that would overflow it is refused).  Between steps only."""
        self._check(self._fn("set_maps")(self.h, int(level), int(block), int(stride), int(records), self._err, ERRLEN))
        self.maps_records = int(records) if level else 0

    def download_maps(self) -> dict:
        """The records held, oldest first, and empties the recorder.  count, tstp[n], block; raw[n, cnt, Mc, Lc] (Mc =
        ceil((mm+1)/B) block rows, Lc = ceil((lm+1)/B) block columns); the views n[n, Mc, Lc] (live cells per block: what a
        mean divides by) and h, u, v [n, nlay, Mc, Lc]; at level >= 2 ke, hu, hv; at level 3 q[n, ntrc, nlay, Mc, Lc]."""
        nl = self.p.nlay
        lv = 0 if self._multi else self.info("maps")                     # (set_tracers with another count frees level 3)
        B = self.info("maps_block") if lv else 1
        Lc, Mc = -(-(self.p.lm + 1) // B), -(-(self.p.mm + 1) // B)
        n, tstp, raw = self._recorder_download("maps", "maps", lv, self.maps_records,
                                               lambda lv: self.lib.beom_maps_count(self.ntrc, nl, lv), Mc * Lc)
        cnt = raw.shape[2]
        raw = raw.reshape(n, cnt, Mc, Lc)           # (a record is [lines * cnt] doubles; inside it is [cnt][Mc][Lc])
        E = 6 if lv >= 2 else 3
        f = raw[:, 1:1 + E * nl].reshape(n, nl, E, Mc, Lc)
        out = {"count": n, "tstp": tstp, "block": B, "raw": raw, "n": raw[:, 0]}
        for m, name in enumerate(("h", "u", "v", "ke", "hu", "hv")[:E]):
            out[name] = f[:, :, m]
        if lv >= 3:
            out["q"] = raw[:, 1 + 6 * nl:].reshape(n, self.ntrc, nl, Mc, Lc)
        return out


class Engine(_Tracers, _Floats, _Moments, _TracerMoments, _Series, _TracerSeries, _ColumnSeries, _TracerColumnSeries, _Maps, _Harmonics, _Forcing):
    """One handle = one GPU's copy of the engine state (mirror of the Fortran module)."""

    _prefix = "beom_"

    def __init__(self, f: Fields, device: int = 0, variant: int = 0, dense_hint: int = 1,
                 upload: bool = True, slab_row0: int = 0, slab_mm: int = 0):
        self.lib = load()
        self.f = f
        self.p = f.p
        self.device = device
        self.prm = make_params_struct(f.p, f, variant, dense_hint, slab_row0, slab_mm)
        self._err = C.create_string_buffer(ERRLEN + 1)
        self.h = C.c_void_p()
        opt = lambda k: _dp(getattr(f, k)) if f.has.get(k, True) else None
        rc = self.lib.beom_create(
            C.byref(self.prm), device, _ip(f.neig), _ip(f.subc),
            _dp(f.mk_u), _dp(f.mk_v), _dp(f.mk_n), _dp(f.mkpe), _dp(f.mkpi),
            _dp(f.fcor), _dp(f.h_th), _dp(f.h_to), _dp(f.nudg), _dp(f.fnud),
            opt("hdot"), opt("tide"), opt("bodf"), _dp(f.taus),
            C.byref(self.h), self._err, ERRLEN)
        self._check(rc)
        if f.flag_nudging and float(f.p.mcbc) < 0.5 and f.segm is not None:     # no_gradient_obc (:2613)
            seg = np.ascontiguousarray(f.segm, dtype=np.int32)
            self._check(self.lib.beom_set_open_boundaries(self.h, seg.shape[1], _ip(seg), self._err, ERRLEN))
        if float(f.p.rgld) > 0.5:                                                # rigid lid: the Poisson operators (:505-563)
            self._check(self.lib.beom_set_rigid_lid(self.h, _dp(f.Ow), _dp(f.Os), _dp(f.Osum_), _dp(f.pi_s),
                                                    self._err, ERRLEN))
        if upload:
            self.upload(**{k: getattr(f, k) for k in STATE_NAMES})

    def upload_pressure(self, pi_s):
        """The lid pressure pi_s(0:ndeg) of a rigid-lid handle (rgld = 1)."""
        self._check(self.lib.beom_set_rigid_lid(self.h, None, None, None, _dp(np.ascontiguousarray(pi_s, dtype=np.float64)),
                                                self._err, ERRLEN))

    def download_pressure(self):
        out = np.zeros(self.p.ndeg + 1)
        self._check(self.lib.beom_download_pressure(self.h, _dp(out), self._err, ERRLEN))
        return out

    def _check(self, rc):
        if rc != 0:
            raise BeomError("beom_hip error %d: %s" % (rc, self._err.value.decode(errors="replace")))

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.beom_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def upload(self, **arrays):
        args = [_dp(arrays.get(k)) for k in STATE_NAMES]
        self._check(self.lib.beom_upload_state(self.h, *args, self._err, ERRLEN))

    def download(self, names=STATE_NAMES) -> dict:
        f = self.f
        out = {k: np.zeros_like(getattr(f, k)) for k in names}
        args = [_dp(out.get(k)) for k in STATE_NAMES]
        self._check(self.lib.beom_download_state(self.h, *args, self._err, ERRLEN))
        return out

    def download_scratch(self) -> dict:
        n1 = self.p.ndeg + 1
        out = {k: np.zeros((self.p.nlay, n1)) for k in SCRATCH_NAMES}
        self._check(self.lib.beom_download_scratch(self.h, *[_dp(out[k]) for k in SCRATCH_NAMES],
                                                   self._err, ERRLEN))
        return out

    def step(self, tstp_first: int, nsteps: int, tres: Optional[float] = None, sync: bool = True):
        p = self.p
        tres = float(getattr(self.f, "tres", 0.0)) if tres is None else tres      # a restarted run continues from its record's time
        self._check(self.lib.beom_step(self.h, tstp_first, nsteps, tres, float(p.dtd8),
                                       float(p.dt_r), float(p.rsta), p.n_3d, self._err, ERRLEN))
        if sync:
            self.sync()

    def sync(self):
        self._check(self.lib.beom_sync(self.h, self._err, ERRLEN))

    def integrals(self) -> dict:
        """Conservation integrals of the state as it stands (beom_integrals): the raw sums and the scaled figures
        (scale_integrals).  Syncs the handle's stream."""
        raw = np.zeros(self.lib.beom_integral_count(self.p.nlay))
        self._check(self.lib.beom_integrals(self.h, _dp(raw), self._err, ERRLEN))
        return scale_integrals(raw, self.prm)

    def integral_rows(self, jlo: int, nrows: int) -> np.ndarray:
        """Row sums [nrows, 4*nlay + 1] of local rows jlo .. jlo+nrows-1 (1-based); combine_integral_rows finishes them."""
        rows = np.zeros((nrows, self.lib.beom_integral_count(self.p.nlay)))
        self._check(self.lib.beom_integral_rows(self.h, jlo, nrows, _dp(rows), self._err, ERRLEN))
        return rows

    def set_stream(self, hip_stream: Optional[int]):
        """hip_stream: integer handle (torch.cuda.current_stream().cuda_stream; 0 = the default
        stream) — or None to go back to the handle's own stream."""
        if hip_stream is None:
            self._check(self.lib.beom_set_stream(self.h, None, 1))
        else:
            self._check(self.lib.beom_set_stream(self.h, C.c_void_p(hip_stream), 0))

    def step_phase(self, tstp: int, phase: int, tres: Optional[float] = None) -> bool:
        """Split step (beom_step_phase).  False if not available for this step."""
        p = self.p
        tres = float(getattr(self.f, "tres", 0.0)) if tres is None else tres
        rc = self.lib.beom_step_phase(self.h, tstp, tres, float(p.dtd8), float(p.dt_r),
                                      float(p.rsta), p.n_3d, phase, self._err, ERRLEN)
        if rc == -20:
            return False
        self._check(rc)
        return True

    def _rows_buffer(self, nrows: int, tensor):
        need = (5 + self.ntrc) * self.p.nlay * nrows * (self.p.lm + 1)      # q of every tracer travels behind the five fields
        if tensor.numel() < need:
            raise BeomError("row buffer of %d elements, %d needed (%d fields)" % (tensor.numel(), need, 5 + self.ntrc))
        return C.c_void_p(tensor.data_ptr())

    def pack_rows(self, jlo: int, nrows: int, tensor):
        self._check(self.lib.beom_pack_rows(self.h, jlo, nrows, self._rows_buffer(nrows, tensor)))

    def unpack_rows(self, jlo: int, nrows: int, tensor):
        self._check(self.lib.beom_unpack_rows(self.h, jlo, nrows, self._rows_buffer(nrows, tensor)))

    def download_outputs(self, h0r4: Optional[np.ndarray]):
        """(eta, u, v) real*4 records [nlay, ndeg], minmax [nlay, 6], thin_layer — formed on the device."""
        n = (self.p.nlay, self.p.ndeg)
        eta, u4, v4 = (np.zeros(n, dtype=np.float32) for _ in range(3))
        mm = np.zeros((self.p.nlay, 6))
        thin = C.c_int(0)
        hp = h0r4.ctypes.data_as(C.c_void_p) if h0r4 is not None else None
        self._check(self.lib.beom_download_outputs(self.h, hp, eta.ctypes.data_as(C.c_void_p),
                                                   u4.ctypes.data_as(C.c_void_p), v4.ctypes.data_as(C.c_void_p),
                                                   _dp(mm), C.byref(thin), self._err, ERRLEN))
        return eta, u4, v4, mm, thin.value

    def download_diag(self):
        """(pvor, mont, v_cc) real*4 records [nlay, ndeg] of write_array's `diag` branch, formed on the device."""
        n = (self.p.nlay, self.p.ndeg)
        out = [np.zeros(n, dtype=np.float32) for _ in range(3)]
        self._check(self.lib.beom_download_diag(self.h, *[a.ctypes.data_as(C.c_void_p) for a in out], self._err, ERRLEN))
        return tuple(out)

    def set_option(self, name: str, value: int):
        self._check(self.lib.beom_set_option(self.h, name.encode(), int(value)))

    def profile_start(self):
        self._check(self.lib.beom_profile_start(self.h))

    def profile_stop(self):
        ms = (C.c_double * 8)()
        nl = (C.c_int * 8)()
        self._check(self.lib.beom_profile_stop(self.h, ms, nl, self._err, ERRLEN))
        return list(ms)[:8], list(nl)[:8]

    def info(self, what: str) -> int:
        """beom_info: "stress_folded" (the last step formed its stress inside the momentum sweep: tt3d, tb3d, tu3d are
        then not kept current), "tile_rows", "biharm_tiled" (1: the handle's biharmonic viscosity, svis > 0, runs as the tiled
        sweep; 0 on the table path and with svis = 0), "uv_fused" (1: the last step's momentum ran as the fused u+v sweep),
        "plain_sweeps" (bit 0: the last step's u+v sweep ran its plain form, bit 1: its Montgomery sweep did),
        "vel_targets_zero" (1: the handle's velocity targets fnud[IX_U], fnud[IX_V] are +0 bit for bit, so the momentum sweeps
        never fetch them for a lane whose velocity is an exact zero), "tracers", "tracer_scheme" (1 upstream, 2 limited),
        "tracer_mixing" (1: set_tracer_mixing is in force), "tracer_mix_launches" (mixing launches so far),
        "tracer_vmixing" (1: set_tracer_vertical_mixing is in force), "tracer_vmix_launches" (its launches so far), "floats",
        "float_records" (records the track recorder holds), "float_launches" (float launches so far), "moments" (the level kept),
        "moment_samples", "moment_launches", "tracer_moments" (the tracer moments' level), "tracer_moment_samples",
        "tracer_moment_launches", "harmonics" (the frequencies fitted), "harmonic_level", "harmonic_samples",
        "harmonic_launches" (one per field and sample), "series" (the series' level), "series_records" (records its recorder holds), "tracer_series" (the tracer series' level),
        "tracer_series_records", "column_series" (the column series' level), "column_series_records",
        "tracer_column_series" (the tracer column series' level), "tracer_column_series_records", "maps" (the maps' level),
        "maps_block" (their block edge), "maps_records", "map_launches" (map launches so far)."""
        v = self.lib.beom_info(self.h, what.encode())
        if v < 0:
            raise BeomError("beom_info(%s) = %d" % (what, v))
        return v

    def field_tensors(self, names=("hlay", "u", "v", "h_u", "h_v")):
        """Zero-copy torch views [nlay, layer stride] of the device-resident prognostic fields.  Handles on the
        table path keep the packed layout (layer stride ndeg+1); dense handles use a padded row pitch — cell
        (i, j) at i + (j-1)*pitch (`self.row_pitch`) — so move rows with pack_rows/unpack_rows, not by slicing."""
        import torch
        out = {}
        cache = self.__dict__.setdefault("_tensor_cache", {})
        for k in names:
            ptr, sl, sr, r0 = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64()
            self._check(self.lib.beom_device_field(self.h, k.encode(), C.byref(ptr), C.byref(sl),
                                                   C.byref(sr), C.byref(r0)))
            n1 = sl.value
            self.row_pitch = sr.value
            t = cache.get(ptr.value)          # the fused sweeps ping-pong buffers: key by address
            if t is None:
                class _Iface:
                    __cuda_array_interface__ = {"shape": (self.p.nlay, n1), "typestr": "<f8",
                                                "data": (ptr.value, False), "version": 3}
                t = cache[ptr.value] = torch.as_tensor(_Iface(), device=torch.device("cuda", self.device))
            out[k] = t
        return out

    def profile_steps(self, tstp_first: int, nsteps: int, tres: Optional[float] = None):
        p = self.p
        tres = float(getattr(self.f, "tres", 0.0)) if tres is None else tres
        ms = (C.c_double * 8)()
        nl = (C.c_int * 8)()
        self._check(self.lib.beom_profile_steps(self.h, tstp_first, nsteps, tres, float(p.dtd8),
                                                float(p.dt_r), float(p.rsta), p.n_3d, ms, nl,
                                                self._err, ERRLEN))
        return list(ms)[:8], list(nl)[:8]

    @property
    def is_dense(self) -> bool:
        """The tiled fast path is active (frames without land, or with land embedded in the rectangle)."""
        return bool(self.lib.beom_is_dense(self.h))

    @property
    def is_embedded(self) -> bool:
        """A frame with land running on the rectangle (masks from arrays in the tiles that touch land)."""
        return self.lib.beom_is_dense(self.h) == 2

    # per-sweep entry points (parity tests)
    def update_h(self, gene, ramp, ctim): self._check(self.lib.beom_update_h(self.h, gene, ramp, ctim))
    def update_tracers(self, gene, ramp, ctim): self._check(self.lib.beom_update_tracers(self.h, gene, ramp, ctim))
    def update_tracer_mixing(self): self._check(self.lib.beom_update_tracer_mixing(self.h))
    def update_tracer_vertical_mixing(self): self._check(self.lib.beom_update_tracer_vmixing(self.h))
    def update_mont(self, ilay=0): self._check(self.lib.beom_update_mont_rvor_pvor_dive_kine(self.h, ilay))
    def update_viscosity(self, ilay=0): self._check(self.lib.beom_update_viscosity(self.h, ilay))
    def update_u(self, ilay, gene, ramp, ctim): self._check(self.lib.beom_update_u(self.h, ilay, gene, ramp, ctim))
    def update_v(self, ilay, gene, ramp, ctim): self._check(self.lib.beom_update_v(self.h, ilay, gene, ramp, ctim))
    def sample_moments(self):
        """Per-sweep entry: one sample of the state as it stands, whatever the stride."""
        self._accum_plain("sample", "moments", "moments")

    def sample_tracer_moments(self):
        """Per-sweep entry: one sample of the tracers and the state as they stand, whatever the stride."""
        self._accum_plain("sample", "tracer_moments", "tracer moments")

    def sample_harmonics(self, ctim: float):
        """Per-sweep entry: one sample at time ctim (days) of the state as it stands, whatever the stride."""
        rc = self.lib.beom_sample_harmonics(self.h, float(ctim))
        if rc != 0:
            raise BeomError("beom_hip error %d: beom_sample_harmonics (harmonics set?)" % rc)

    def sample_series(self):
        """Per-sweep entry: one record of the fields as they stand, under the last step's number, whatever the stride."""
        self._recorder_sample("series", "series")

    def sample_column_series(self):
        """One record of the column series by hand, of the fields as they stand, under the last step's number."""
        self._recorder_sample("column_series", "column series")

    def sample_tracer_column_series(self):
        """One record of the tracer column series by hand, of the tracers and the state as they stand, under the last step's
        number."""
        self._recorder_sample("tracer_column_series", "tracer column series")

    def sample_maps(self):
        """One record of the maps by hand, of the fields as they stand, under the last step's number."""
        self._recorder_sample("maps", "maps")

    def sample_tracer_series(self):
        """Per-sweep entry: one record of the tracers and the state as they stand, under the last step's number, whatever the
        stride."""
        self._recorder_sample("tracer_series", "tracer series")

    def rebuild_fluxes(self): self._check(self.lib.beom_rebuild_fluxes(self.h))
    def distribute_stress(self): self._check(self.lib.beom_distribute_stress(self.h))


class MultiEngine(_Tracers, _Floats, _Moments, _TracerMoments, _Series, _TracerSeries, _ColumnSeries, _TracerColumnSeries, _Maps, _Harmonics, _Forcing):
    """beom_multi_*: the whole frame on several HIP devices from ONE process (row bands with ghost
    exchange inside the library) — what the Fortran host uses with BEOM_NGPU > 1.  `devices` may
    name a device more than once (tests: three bands on the one GPU of the box)."""

    def __init__(self, f: Fields, devices=(0,), variant: int = 0, upload: bool = True,
                 transport: int = XCHG_PEER, ring1: bool = False):
        self.lib = load()
        self.f, self.p = f, f.p
        self.prm = make_params_struct(f.p, f, variant, 1, 0, 0)
        self._err = C.create_string_buffer(ERRLEN + 1)
        self.h = C.c_void_p()
        dev = (C.c_int * len(devices))(*devices)
        opt = lambda k: _dp(getattr(f, k)) if f.has.get(k, True) else None
        rc = self.lib.beom_multi_create_ex(
            C.byref(self.prm), len(devices), dev, transport | (XCHG_RING1 if ring1 else 0), _ip(f.neig), _ip(f.subc),
            _dp(f.mk_u), _dp(f.mk_v), _dp(f.mk_n), _dp(f.mkpe), _dp(f.mkpi),
            _dp(f.fcor), _dp(f.h_th), _dp(f.h_to), _dp(f.nudg), _dp(f.fnud),
            opt("hdot"), opt("tide"), opt("bodf"), _dp(f.taus),
            C.byref(self.h), self._err, ERRLEN)
        self._check(rc)
        if f.flag_nudging and float(f.p.mcbc) < 0.5 and f.segm is not None:     # no_gradient_obc (:2613), dealt to the bands
            seg = np.ascontiguousarray(f.segm, dtype=np.int32)
            self._check(self.lib.beom_multi_set_open_boundaries(self.h, seg.shape[1], _ip(seg), self._err, ERRLEN))
        if upload:
            self.upload(**{k: getattr(f, k) for k in STATE_NAMES})

    _check = Engine._check
    _prefix = "beom_multi_"

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            self.lib.beom_multi_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def count(self) -> int:
        return self.lib.beom_multi_count(self.h)

    def band(self, k: int) -> dict:
        v = [C.c_int() for _ in range(5)]
        self._check(self.lib.beom_multi_band(self.h, k, *[C.byref(x) for x in v]))
        return dict(zip(("own0", "own1", "win0", "win1", "device"), (x.value for x in v)))

    def upload(self, **arrays):
        args = [_dp(arrays.get(k)) for k in STATE_NAMES]
        self._check(self.lib.beom_multi_upload_state(self.h, *args, self._err, ERRLEN))

    def download(self, names=STATE_NAMES) -> dict:
        out = {k: np.zeros_like(getattr(self.f, k)) for k in names}
        args = [_dp(out.get(k)) for k in STATE_NAMES]
        self._check(self.lib.beom_multi_download_state(self.h, *args, self._err, ERRLEN))
        return out

    def step(self, tstp_first: int, nsteps: int, tres: Optional[float] = None, sync: bool = True):
        p = self.p
        tres = float(getattr(self.f, "tres", 0.0)) if tres is None else tres      # a restarted run continues from its record's time
        self._check(self.lib.beom_multi_step(self.h, tstp_first, nsteps, tres, float(p.dtd8), float(p.dt_r),
                                             float(p.rsta), p.n_3d, self._err, ERRLEN))
        if sync:
            self.sync()

    def sync(self):
        self._check(self.lib.beom_multi_sync(self.h, self._err, ERRLEN))

    def integrals(self) -> dict:
        """As Engine.integrals: every band forms the row sums of its owned rows; the same bits as the single handle's."""
        raw = np.zeros(self.lib.beom_integral_count(self.p.nlay))
        self._check(self.lib.beom_multi_integrals(self.h, _dp(raw), self._err, ERRLEN))
        return scale_integrals(raw, self.prm)

    def stats(self) -> dict:
        a, b = C.c_longlong(), C.c_longlong()
        self.lib.beom_multi_stats(self.h, C.byref(a), C.byref(b))
        return {"split": a.value, "plain": b.value}

    def download_outputs(self, h0r4: np.ndarray):
        """(eta, u, v) real*4 records [nlay, ndeg], minmax [nlay, 6], thin_layer — every band forms its rows on its device."""
        n = (self.p.nlay, self.p.ndeg)
        eta, u4, v4 = (np.zeros(n, dtype=np.float32) for _ in range(3))
        mm = np.zeros((self.p.nlay, 6))
        thin = C.c_int(0)
        self._check(self.lib.beom_multi_download_outputs(self.h, h0r4.ctypes.data_as(C.c_void_p), eta.ctypes.data_as(C.c_void_p),
                                                         u4.ctypes.data_as(C.c_void_p), v4.ctypes.data_as(C.c_void_p),
                                                         _dp(mm), C.byref(thin), self._err, ERRLEN))
        return eta, u4, v4, mm, thin.value

    def download_diag(self):
        n = (self.p.nlay, self.p.ndeg)
        out = [np.zeros(n, dtype=np.float32) for _ in range(3)]
        self._check(self.lib.beom_multi_download_diag(self.h, *[a.ctypes.data_as(C.c_void_p) for a in out], self._err, ERRLEN))
        return tuple(out)

    def describe(self) -> dict:
        v = [C.c_int() for _ in range(5)]
        self._check(self.lib.beom_multi_describe(self.h, *[C.byref(x) for x in v]))
        d = dict(zip(("bands_total", "bands_local", "transport", "ring", "rccl_version"), (x.value for x in v)))
        d["transport"] = {XCHG_PEER: "hipMemcpyPeerAsync", XCHG_RCCL: "RCCL ncclSend/ncclRecv",
                          XCHG_SHM: "POSIX shared memory (host-staged)"}.get(d["transport"], "?")
        return d

    def profile_start(self):
        self._check(self.lib.beom_multi_profile_start(self.h))

    def profile_stop(self):
        ms = (C.c_double * 8)()
        nl = (C.c_int * 8)()
        self._check(self.lib.beom_multi_profile_stop(self.h, ms, nl, self._err, ERRLEN))
        return list(ms)[:8], list(nl)[:8]

    def profile_steps(self, tstp_first: int, nsteps: int, tres: Optional[float] = None):
        self.profile_start()
        self.step(tstp_first, nsteps, tres, sync=False)
        return self.profile_stop()

    def set_option(self, name: str, value: int):
        """"overlap": split steps around the exchange in flight; other names go to every band."""
        self._check(self.lib.beom_multi_set_option(self.h, name.encode(), int(value)))

    def info(self, what: str) -> int:
        """beom_info of band 0's handle (all bands of a frame run the same launches); "float_handovers": the records ingested
        so far, summed over the bands, as the latest download_floats read them."""
        bands = range(self.count) if what == "float_handovers" else (0,)
        total = 0
        for k in bands:
            v = self.lib.beom_info(self.band_engine_handle(k), what.encode())
            if v < 0:
                raise BeomError("beom_info(%s) = %d" % (what, v))
            total += v
        return total

    def band_engine_handle(self, k: int) -> C.c_void_p:
        h = C.c_void_p()
        self._check(self.lib.beom_multi_engine(self.h, k, C.byref(h)))
        return h


def device_pci_bus_id(device: int) -> Optional[str]:
    buf = C.create_string_buffer(64)
    return buf.value.decode().lower() if load().beom_device_pci_bus_id(device, buf, 64) == 0 else None


def rccl_unique_id() -> bytes:
    """128 bytes of ncclGetUniqueId (one rank calls it, every rank of the job gets the bytes)."""
    lib = load()
    buf = C.create_string_buffer(128)
    err = C.create_string_buffer(ERRLEN + 1)
    rc = lib.beom_rccl_unique_id(buf, err, ERRLEN)
    if rc != 0:
        raise BeomError("beom_rccl_unique_id %d: %s" % (rc, err.value.decode(errors="replace")))
    return buf.raw


def multi_window(p: Params, nb: int, band: int, yper: bool) -> dict:
    """Rows of band `band` of `nb`: owned global rows own0..own1 and the ghost rows on either side."""
    lib = load()
    prm = make_params_struct(p)
    v = [C.c_int() for _ in range(4)]
    rc = lib.beom_multi_window(C.byref(prm), nb, band, int(bool(yper)), *[C.byref(x) for x in v])
    if rc != 0:
        raise BeomError("beom_multi_window %d" % rc)
    return dict(zip(("own0", "own1", "ghost_s", "ghost_n"), (x.value for x in v)))


class BandEngine(MultiEngine):
    """beom_multi_create_local[_ex]: ONE band of a frame cut over `nb` processes, built from that band's window
    only (bench.py under torchrun; exchange over RCCL).  `f` = the window's Fields (rows: south ghosts,
    owned rows, north ghosts — beom_amd.slab.build_window), `p_global` the global frame's parameters,
    `orphan` = Fields of row mm+1 (band 0 of a frame periodic in y).  `shm_name` ("/...", the same on every
    rank) selects the shared-memory transport instead of RCCL: ranks of one node that may share a device;
    `loopback`: the band receives its own sends (one band alone with the whole exchange machinery: timing)."""

    def __init__(self, f: Fields, p_global: Params, nb: int, band: int, device: int = 0, variant: int = 0,
                 rccl_id: Optional[bytes] = None, orphan: Optional[Fields] = None, upload: bool = True,
                 shm_name: Optional[str] = None, loopback: bool = False):
        self.lib = load()
        self.f, self.p, self.pg = f, f.p, p_global
        self.orphan = orphan
        self.prm = make_params_struct(p_global, f, variant, 1, 0, 0)
        self._err = C.create_string_buffer(ERRLEN + 1)
        self.h = C.c_void_p()
        if shm_name is not None:
            idbuf, transport = C.create_string_buffer(shm_name.encode()), XCHG_SHM
        else:
            idbuf, transport = (C.create_string_buffer(rccl_id, 128) if rccl_id is not None else None), XCHG_RCCL
        st = self._statics(f)
        so = self._statics(orphan) if orphan is not None else None
        rc = self.lib.beom_multi_create_local_ex(
            C.byref(self.prm), nb, band, device, int(float(p_global.xper) > 0.5), int(float(p_global.yper) > 0.5),
            transport | (XCHG_LOOPBACK if loopback else 0), idbuf, C.byref(st), C.byref(so) if so is not None else None,
            C.byref(self.h), self._err, ERRLEN)
        self._check(rc)
        if bool(f.flag_nudging) and float(p_global.mcbc) < 0.5:       # no_gradient_obc (:2613): the segments of this window's rows
            seg = lambda x: np.ascontiguousarray(x.segm, dtype=np.int32) if (x is not None and x.segm is not None) else None
            sw, so_ = seg(f), seg(orphan)
            self._check(self.lib.beom_multi_set_open_boundaries_local(
                self.h, 0 if sw is None else sw.shape[1], None if sw is None else _ip(sw),
                0 if so_ is None else so_.shape[1], None if so_ is None else _ip(so_), self._err, ERRLEN))
        if upload:
            self.upload()

    @staticmethod
    def _statics(f: Fields) -> BeomStatics:
        s = BeomStatics()
        for k in STATICS_NAMES:
            present = f.has.get(k, True) if k in ("hdot", "tide", "bodf") else True
            setattr(s, k, _dp(getattr(f, k)) if present else None)
        return s

    @staticmethod
    def _state(arrays: dict) -> BeomState:
        s = BeomState()
        for k in STATE_NAMES:
            setattr(s, k, _dp(arrays.get(k)))
        return s

    def upload(self, **arrays):
        src = arrays or {k: getattr(self.f, k) for k in STATE_NAMES}
        sw = self._state(src)
        so = self._state({k: getattr(self.orphan, k) for k in STATE_NAMES}) if self.orphan is not None else None
        self._check(self.lib.beom_multi_upload_local(self.h, C.byref(sw), C.byref(so) if so is not None else None,
                                                     self._err, ERRLEN))

    def integrals(self) -> dict:
        raise BeomError("a band holds a window: gather integral_rows() of all bands and combine_integral_rows them")

    def integral_rows(self):
        """(own0, own1, rows[own1-own0+1, 4*nlay + 1]): the row sums of this band's owned global rows.  The caller stacks the
        bands' rows in global row order (row mm+1 of a frame periodic in y: zeros) for combine_integral_rows."""
        w = self.band(0)
        rows = np.zeros((w["own1"] - w["own0"] + 1, self.lib.beom_integral_count(self.pg.nlay)))
        a, b = C.c_int(), C.c_int()
        self._check(self.lib.beom_multi_integral_rows_local(self.h, C.byref(a), C.byref(b), _dp(rows), self._err, ERRLEN))
        return a.value, b.value, rows

    def download(self, names=STATE_NAMES, orphan: bool = False) -> dict:
        out = {k: np.zeros_like(getattr(self.f, k)) for k in names}
        sw = self._state(out)
        oo, so = None, None
        if orphan and self.orphan is not None:
            oo = {k: np.zeros_like(getattr(self.orphan, k)) for k in names}
            so = self._state(oo)
        self._check(self.lib.beom_multi_download_local(self.h, C.byref(sw), C.byref(so) if so is not None else None,
                                                       self._err, ERRLEN))
        return (out, oo) if orphan else out
