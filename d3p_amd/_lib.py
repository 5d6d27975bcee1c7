"""ctypes binding of libd3p_hip.so (C-ABI declared in include/d3p_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``d3p_amd._lib.build()`` with
``hipcc --offload-arch=gfx950``.  There is no CPU fallback: if the shared object is missing, or no
HIP device is visible, every compute entry point raises.
"""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libd3p_hip.so")
_SRC = [os.path.join(_HERE, "csrc", f) for f in ("d3p_rng.hip", "d3p_dpvi.hip", "d3p_stages.hip", "d3p_gmm.hip", "d3p_gemm.hip", "d3p_vae.hip", "d3p_fmesh.hip", "d3p_predict.hip", "d3p_loglik.hip", "d3p_moments.hip", "d3p_predict_glm.hip", "d3p_predict_gmm.hip", "d3p_gmm_density.hip", "d3p_psis.hip", "d3p_draw_sums.hip", "d3p_vae_density.hip", "d3p_quantiles.hip", "d3p_grad_norms.hip", "d3p_hpdi.hip", "d3p_crps.hip", "d3p_model_weights.hip", "d3p_rep_stats.hip", "d3p_discrepancy.hip", "d3p_classify.hip", "d3p_energy.hip", "d3p_pair_stats.hip", "d3p_marginals.hip", "d3p_label_sums.hip")]
_DEPS = _SRC + [os.path.join(_HERE, "csrc", f) for f in ("d3p_device.h", "d3p_host.h", "d3p_glm_tile.h", "d3p_outcome.h", "d3p_row_sums.h", "d3p_pair_tile.h", "d3p_shifted_sums.h", "d3p_colreduce.h", "d3p_colsort.h", "d3p_crps.h", "d3p_crps_kernel.h", "d3p_gemm.h", "d3p_logreg_kernel.h", "d3p_logreg_chain.h", "d3p_logreg_persist.h", "d3p_logreg_wide.h", "d3p_logreg_particles.h", "d3p_fmesh.h", "d3p_ipc_arena.h")] + [
    os.path.join(os.path.dirname(_HERE), "include", "d3p_hip.h")]

D3P_BATCH_EXPLICIT, D3P_BATCH_FEISTEL, D3P_BATCH_POISSON = 0, 1, 2
D3P_FAMILY_LOGREG, D3P_FAMILY_GAUSS_MEAN, D3P_FAMILY_LINREG, D3P_FAMILY_POISSON = 0, 1, 2, 3
D3P_GUIDE_SOFTPLUS, D3P_GUIDE_EXP, D3P_GUIDE_EXP_SITES = 0, 1, 2


class D3PError(RuntimeError):
    pass


class LogregModel(C.Structure):
    _fields_ = [("d", C.c_int32), ("intercept", C.c_int32), ("prior_w", C.c_float),
                ("prior_b", C.c_float), ("lik_scale", C.c_float), ("inv_obs", C.c_float),
                ("family", C.c_int32), ("guide_transform", C.c_int32), ("lik_sigma", C.c_float)]


class GmmModel(C.Structure):
    _fields_ = [("K", C.c_int32), ("d", C.c_int32), ("prior_mu_scale", C.c_float), ("lik_scale", C.c_float),
                ("inv_obs", C.c_float)]


class VaeModel(C.Structure):
    _fields_ = [("D", C.c_int32), ("H", C.c_int32), ("Z", C.c_int32), ("scale", C.c_float), ("inv_obs", C.c_float),
                ("H2", C.c_int32)]   # H2 > 0: a second hidden layer on each side (BASELINE config 5's [400, 200] variant)


class GemmOpts(C.Structure):
    """d3p_gemm_opts (include/d3p_hip.h, test aids): the options of the VAE's product dispatcher."""
    _fields_ = [("a_last_one", C.c_int32), ("epi", C.c_int32), ("part", C.c_void_p), ("part_floats", C.c_uint64), ("C2", C.c_void_p),
                ("ex_zu", C.c_void_p), ("ex_eps", C.c_void_p), ("ep_x", C.c_void_p), ("ep_ll", C.c_void_p), ("ep_xx", C.c_void_p),
                ("ex_Z", C.c_int32), ("ex_sc", C.c_float), ("has_jumps", C.c_int32), ("n_seg", C.c_int32), ("k_seg", C.c_int32),
                ("force_splits", C.c_int32), ("b_njump", C.c_int64), ("b_kjump", C.c_int64), ("bias_njump", C.c_int64),
                ("c_njump", C.c_int64), ("b_row_scale", C.c_void_p), ("exact16_word", C.c_void_p), ("exact16_nonce", C.c_uint32),
                ("leave_split", C.c_int32)]


class GemmReport(C.Structure):
    _fields_ = [("route", C.c_int32), ("splits", C.c_int32), ("splits_left", C.c_int32)]


class GemmMember(C.Structure):
    """d3p_gemm_member: one product of d3p_gemm_f32_group."""
    _fields_ = [("A", C.c_void_p), ("a_sm", C.c_int64), ("a_sk", C.c_int64), ("B", C.c_void_p), ("b_sk", C.c_int64), ("b_sn", C.c_int64),
                ("C", C.c_void_p), ("bias", C.c_void_p), ("ldc", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("alpha", C.c_float), ("accumulate", C.c_int32), ("opts", GemmOpts), ("report", GemmReport), ("joined", C.c_int32)]


D3P_GROUP_MAX = 6
GEMM_ROUTE_F32, GEMM_ROUTE_F32_VA, GEMM_ROUTE_F32_VB, GEMM_ROUTE_W8, GEMM_ROUTE_BF16X3, GEMM_ROUTE_GROUPED = 0, 1, 2, 4, 5, 6


class PredictSite(C.Structure):
    """d3p_predict_site (include/d3p_hip.h): one latent sample site of the predictive draws."""
    _fields_ = [("size", C.c_int32), ("offset", C.c_int32), ("chain", C.c_int32), ("key_index", C.c_int32),
                ("scale_kind", C.c_int32), ("loc_c", C.c_float), ("scale_c", C.c_float), ("loc_dev", C.c_void_p),
                ("scale_dev", C.c_void_p), ("value_dev", C.c_void_p)]


D3P_PREDICT_SCALE_CONST, D3P_PREDICT_SCALE_GIVEN, D3P_PREDICT_SCALE_EXP = 0, 1, 2


class DpsviHyper(C.Structure):
    _fields_ = [("clip", C.c_float), ("dp_scale", C.c_float), ("lr", C.c_float),
                ("b1", C.c_float), ("b2", C.c_float), ("adam_eps", C.c_float)]


class DpsviState(C.Structure):
    _fields_ = [("rng_key", C.c_void_p), ("key_slot", C.c_int32), ("params", C.c_void_p),
                ("adam_m", C.c_void_p), ("adam_v", C.c_void_p), ("step", C.c_void_p)]


class BatchSource(C.Structure):
    _fields_ = [("kind", C.c_int32), ("B", C.c_uint32), ("q", C.c_float), ("suppress", C.c_int32),
                ("batch_key", C.c_void_p), ("batch_index", C.c_void_p), ("mask", C.c_void_p),
                ("n_rows", C.c_uint64), ("row_lo", C.c_uint64), ("row_hi", C.c_uint64)]


_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"]


def _digest(paths):
    """sha256 over the compile flags and the CONTENTS of `paths` (in order)."""
    import hashlib
    h = hashlib.sha256(" ".join(_FLAGS).encode())
    for p in paths:
        h.update(os.path.basename(p).encode() + b"\0")
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def _read(path):
    try:
        with open(path) as f:
            return f.read().strip()
    except OSError:
        return ""


def build(force=False, verbose=False):
    """Compile libd3p_hip.so for gfx950 (hipcc cross-compiles without a GPU): one object per source under build/, then one
    link.  Staleness is decided by CONTENT, not by modification times (a snapshot pushed to another machine need not preserve
    them): the library carries `libd3p_hip.so.srchash` = sha256 of flags + every source and header, every object a digest of
    its source + the headers; whatever does not match is rebuilt (the compiles run in parallel)."""
    want = _digest(_DEPS)
    stamp = _SO + ".srchash"
    if not force and os.path.exists(_SO) and _read(stamp) == want:
        return _SO
    objdir = os.path.join(os.path.dirname(_HERE), "build", "d3p_hip")
    os.makedirs(objdir, exist_ok=True)
    headers = [p for p in _DEPS if p not in _SRC]
    jobs, objs = [], []
    for src in _SRC:
        obj = os.path.join(objdir, os.path.basename(src) + ".o")
        objs.append(obj)
        obj_want = _digest([src] + headers)
        if force or not os.path.exists(obj) or _read(obj + ".srchash") != obj_want:
            cmd = ["hipcc"] + _FLAGS + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            jobs.append((cmd, subprocess.Popen(cmd), obj, obj_want))
    for cmd, proc, obj, obj_want in jobs:
        if proc.wait() != 0:
            raise subprocess.CalledProcessError(proc.returncode, cmd)
        with open(obj + ".srchash", "w") as f:
            f.write(obj_want + "\n")
    cmd = ["hipcc", "--offload-arch=gfx950", "-fPIC", "-shared", "-o", _SO] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    with open(stamp, "w") as f:
        f.write(want + "\n")
    return _SO


def is_stale():
    """True when libd3p_hip.so is missing or was not built from the sources in this tree (content digest)."""
    return not os.path.exists(_SO) or _read(_SO + ".srchash") != _digest(_DEPS)


_V, _U64, _U32, _I32, _F, _SZ = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32, C.c_float, C.c_size_t
_PM, _PH, _PS, _PB = C.POINTER(LogregModel), C.POINTER(DpsviHyper), C.POINTER(DpsviState), C.POINTER(BatchSource)

# name -> (restype, argtypes); every symbol include/d3p_hip.h declares
SIGNATURES = {
    "d3p_abi_version": (C.c_int, []),
    "d3p_last_error": (C.c_char_p, []),
    "d3p_device_count": (C.c_int, []),
    "d3p_rng_split": (C.c_int, [_V, _V, C.c_int, _V]),
    "d3p_key_chain_host": (C.c_int, [_V, C.c_int, _V]),
    "d3p_rng_fold_in": (C.c_int, [_V, _V, _U32, _V]),
    "d3p_rng_random_bits": (C.c_int, [_V, _V, C.c_int, _U64, _V]),
    "d3p_rng_uniform": (C.c_int, [_V, _V, _U64, _F, _F, _V]),
    "d3p_rng_normal": (C.c_int, [_V, _V, _U64, _V]),
    "d3p_rng_randint": (C.c_int, [_V, _V, _U64, _I32, _I32, _V]),
    "d3p_rng_randint_bits": (C.c_int, [_V, _V, _U64, C.c_int, C.c_int64, C.c_int64, _V]),
    "d3p_tf_split": (C.c_int, [_V, _V, C.c_int, _V]),
    "d3p_tf_fold_in": (C.c_int, [_V, _V, _U32, _V]),
    "d3p_tf_random_bits": (C.c_int, [_V, _V, _U64, _V]),
    "d3p_tf_uniform": (C.c_int, [_V, _V, _U64, _F, _F, _V]),
    "d3p_tf_normal": (C.c_int, [_V, _V, _U64, _V]),
    "d3p_tf_randint": (C.c_int, [_V, _V, _U64, _I32, _I32, _V]),
    "d3p_logreg_evaluate_workspace": (_SZ, [_PM, _U32]),
    "d3p_logreg_evaluate": (C.c_int, [_V, _PM, _V, _V, _V, _U32, _V, _V, _V, _SZ]),
    "d3p_logreg_evaluate_sites": (C.c_int, [_V, _PM, _V, _V, _V, _U32, _V, C.POINTER(C.c_int32), _I32, _V, _V, _SZ]),
    "d3p_gmm_log_prob": (C.c_int, [_V, _V, _U32, _I32, _V, _V, _V, _I32, _V]),
    "d3p_feistel_sample": (C.c_int, [_V, _V, _U32, _U32, _V]),
    "d3p_feistel_from_constants": (C.c_int, [_V, _V, _U32, _U32, _V]),
    "d3p_poisson_select_rng": (C.c_int, [_V, C.c_int, _V, _F, _U32, _U32, C.c_int, _V, _V, _V, _SZ]),
    "d3p_poisson_select_batch": (C.c_int, [_V, C.c_int, _V, _SZ, _F, _U32, _U32, C.c_int, _V, _SZ, _V, _SZ, _U32, _V, _SZ]),
    "d3p_poisson_shard_flags": (C.c_int, [_V, C.c_int, _V, _SZ, _F, _U32, _U32, _U32, _U32, _V, _V, _SZ]),
    "d3p_poisson_shard_write": (C.c_int, [_V, _U32, _U32, _U32, _U32, _V, _SZ, _V, _V, _V, _SZ, _U32, _V, _SZ]),
    "d3p_xchg_poisson_counts": (C.c_int, [_V, _V, _V, _U32, _U32, C.c_int, _V, _SZ, _V, _V, _SZ]),
    "d3p_perturb_apply": (C.c_int, [_V, _V, _V, _U64, _F, _F, _V, _F, _V]),
    "d3p_poisson_select_workspace": (_SZ, [_U32]),
    "d3p_poisson_select": (C.c_int, [_V, _V, _F, _U32, _U32, C.c_int, _V, _V, _V, _SZ]),
    "d3p_take_rows": (C.c_int, [_V, _V, _U64, _U32, _V, _U32, _V, _V]),
    "d3p_logreg_px_grads_workspace": (_SZ, [_PM, _U32]),
    "d3p_logreg_px_grads": (C.c_int, [_V, _PM, _V, _V, _V, _V, _U32, _V, _V, _V, _V, _V, _V, _SZ]),
    "d3p_clip_rows": (C.c_int, [_V, _V, _U32, _U32, _F]),
    "d3p_full_norm": (C.c_int, [_V, _V, _U64, _V, _V, _SZ]),
    "d3p_full_norm_ord": (C.c_int, [_V, _V, _U64, C.c_double, _V]),
    "d3p_combine": (C.c_int, [_V, _V, _V, _U32, _U32, _V, _V]),
    "d3p_perturb": (C.c_int, [_V, _V, _V, C.POINTER(C.c_int32), C.c_int, _F, _F, _V, _F, _V, _V]),
    "d3p_adam_step": (C.c_int, [_V, _V, _V, _V, _V, _V, _U32, _F, _F, _F, _F]),
    "d3p_sgd_step": (C.c_int, [_V, _V, _V, _V, _U32, _F]),
    "d3p_gmm_px_grads_workspace": (C.c_size_t, [_I32, _U32]),
    "d3p_gmm_evaluate_workspace": (C.c_size_t, [_V, _U32]),
    "d3p_gmm_evaluate": (C.c_int, [_V, _V, _V, _V, _U32, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_gmm_workspace": (C.c_size_t, [_V, _U32]),
    "d3p_dpvi_gmm_update": (C.c_int, [_V, _V, _V, _V, _V, _V, _U32, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_gmm_run": (C.c_int, [_V, _V, _V, _V, _V, _U32, _V, _U32, _U32, _U32, _V, _V, C.c_size_t]),
    "d3p_gmm_px_grads": (C.c_int, [_V, _V, _V, _V, _V, _U32, _V, _V, _V, _V, _V, _V, C.c_size_t]),
    "d3p_vae_num_params": (C.c_int64, [_V]),
    "d3p_dpvi_vae_workspace": (C.c_size_t, [_V, _U32]),
    "d3p_gemm_f32": (C.c_int, [_V, _V, C.c_int64, C.c_int64, _V, C.c_int64, C.c_int64, _V, _I32, _I32, _I32, _I32, _V, _F, _I32]),
    # test aids: the dispatcher's options and the grouped launch on their own (tests/test_gpu_vae_gemm.py): added symbols, ABI 9 unchanged
    "d3p_gemm_f32_ex": (C.c_int, [_V, _V, C.c_int64, C.c_int64, _V, C.c_int64, C.c_int64, _V, _I32, _I32, _I32, _I32, _V, _F, _I32,
                                  C.POINTER(GemmOpts), C.POINTER(GemmReport)]),
    "d3p_gemm_f32_group": (C.c_int, [_V, C.POINTER(GemmMember), _I32, _I32, _V, _V, _U32]),
    "d3p_vae_step_sums": (C.c_int, [_V, _V, _V, _V, _V, _U32, _V, _V, _F, _V, _V, _V, _V, C.c_size_t]),
    "d3p_vae_evaluate": (C.c_int, [_V, _V, _V, _V, _U32, _V, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_vae_update": (C.c_int, [_V, _V, _V, _V, _V, _V, _U32, _V, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_vae_update_from": (C.c_int, [_V, _V, _V, _V, _V, _V, _V, _U32, _V, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_vae_run": (C.c_int, [_V, _V, _V, _V, _V, _U32, _V, _U32, _U32, _U32, _V, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_gmm_local_sums": (C.c_int, [_V, _V, _V, _V, _V, _V, _U32, _U32, _U32, _V, _V, C.c_size_t]),
    "d3p_dpvi_gmm_apply": (C.c_int, [_V, _V, _V, _V, _V, _U32, _U32, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_vae_local_sums": (C.c_int, [_V, _V, _V, _V, _V, _V, _U32, _U32, _U32, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_vae_apply": (C.c_int, [_V, _V, _V, _V, _V, _U32, _U32, _V, _V, _V, C.c_size_t]),
    "d3p_dpvi_vae_run_dist": (C.c_int, [_V, _V, _V, _V, _V, _V, _V, _V, _U32, _U32, _U32, _U32, _V, C.c_int32, _V, C.c_size_t]),
    "d3p_fmesh_create": (C.c_int, [C.c_int32, C.c_int32, C.c_uint64, _V, _V, C.c_size_t]),
    "d3p_fmesh_connect": (C.c_int, [_V, _V, C.c_size_t]),
    "d3p_fmesh_connect_local": (C.c_int, [_V, _V, C.c_int32]),
    "d3p_fmesh_set_grid": (C.c_int, [_V, C.c_int32]),
    "d3p_fmesh_allreduce": (C.c_int, [_V, _V, _V, C.c_uint64]),
    "d3p_fmesh_status": (C.c_int, [_V, _V, _V]),
    "d3p_fmesh_destroy": (C.c_int, [_V]),
    "d3p_fmesh_disconnect": (C.c_int, [_V]),
    "d3p_dpvi_logreg_chain_status": (C.c_int, [_V, _V, _V, _V, C.c_size_t, _V]),
    "d3p_dpvi_logreg_run_status": (C.c_int, [_V, _V, _V, _V, C.c_size_t, _V, _V]),
    "d3p_xchg_create": (C.c_int, [_I32, _I32, _U32, _V, _V, _SZ]),
    "d3p_xchg_connect": (C.c_int, [_V, _V, _SZ]),
    "d3p_xchg_connect_local": (C.c_int, [_V, _V, _I32]),
    "d3p_xchg_destroy": (C.c_int, [_V]),
    "d3p_xchg_disconnect": (C.c_int, [_V]),
    "d3p_xchg_allreduce": (C.c_int, [_V, _V, _V, _I32]),
    "d3p_xchg_simulate_peers": (C.c_int, [_V, _V, _U32]),
    "d3p_dpvi_logreg_run_xchg": (C.c_int, [_V, _V, _PM, _PH, _PS, _PB, _V, _V, _U32, _V, _V, _SZ]),
    "d3p_dpvi_logreg_set_run_form": (C.c_int, [C.c_int]),
    "d3p_dpvi_logreg_chain_grid": (C.c_int, [_V, _V, C.c_int, _V, _V]),
    "d3p_dpvi_logreg_kernel_timing_enable": (C.c_int, [C.c_int]),
    "d3p_dpvi_logreg_kernel_timing_read": (C.c_int, [_V, _V, _V]),
    "d3p_comm_unique_id": (C.c_int, [_V, C.c_size_t]),
    "d3p_comm_init": (C.c_int, [_V, C.c_size_t, _I32, _I32, _V]),
    "d3p_comm_destroy": (C.c_int, [_V]),
    "d3p_dpvi_logreg_run_dist": (C.c_int, [_V, _V, _V, _V, _V, _V, _V, _V, _U32, _V, _V, C.c_size_t]),
    "d3p_adadp_workspace": (C.c_size_t, []),
    "d3p_adadp_step": (C.c_int, [_V, _V, _V, _V, _V, _V, _V, _U32, _F, C.c_int, _V, C.c_size_t]),
    "d3p_dpvi_logreg_workspace": (_SZ, [_PM, _PB]),
    "d3p_dpvi_logreg_local_sums": (C.c_int, [_V, _PM, _PH, _PS, _PB, _V, _V, _V, _V, _V, _SZ]),
    "d3p_dpvi_logreg_finalize": (C.c_int, [_V, _PM, _PH, _PS, _PB, _V, _V, _V, _V, _SZ]),
    "d3p_dpvi_logreg_begin": (C.c_int, [_V, _PM, _PH, _PS, _PB, _V, _SZ]),
    "d3p_dpvi_logreg_prepare": (C.c_int, [_V, _PM, _PH, _PS, _PB, _U32, _V, _SZ]),
    "d3p_dpvi_logreg_step_sums": (C.c_int, [_V, _PM, _PH, _PS, _PB, _U32, _V, _V, _V, _V, _V, _SZ]),
    "d3p_dpvi_logreg_step_finalize": (C.c_int, [_V, _PM, _PH, _PS, _PB, _U32, _V, _V, _V, _V, _SZ]),
    "d3p_dpvi_logreg_end": (C.c_int, [_V, _PM, _PH, _PS, _PB, _U32, _V, _SZ]),
    "d3p_dpvi_logreg_prepare_buf": (C.c_int, [_V, _PM, _PH, _PS, _PB, _U32, C.c_int, _V, _SZ]),
    "d3p_dpvi_logreg_acc_layout": (C.c_int, [_PM, _PB, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "d3p_dpvi_logreg_acc_reset": (C.c_int, [_V, _PM, _PH, _PS, _PB, _V, _SZ]),
    "d3p_dpvi_logreg_fused_step_supported": (C.c_int, [_PM, _PB]),
    "d3p_dpvi_logreg_fused_step": (C.c_int, [_V, _PM, _PH, _PS, _PB, _U32, _U32, C.c_int, C.c_int, _U32, C.c_int, _V, _V,
                                             _V, C.c_int, _V, _SZ]),
    "d3p_dpvi_logreg_run": (C.c_int, [_V, _PM, _PH, _PS, _PB, _V, _V, _U32, _V, _V, _SZ]),
    "d3p_dpvi_logreg_run_from": (C.c_int, [_V, _PM, _PH, _PS, _PS, _PB, _U32, _V, _V, _U32, _V, _V, _SZ]),
    "d3p_dpvi_logreg_run_dist_from": (C.c_int, [_V, _V, _V, _PM, _PH, _PS, _PS, _PB, _U32, _V, _V, _U32, _V, _V, _SZ]),
    "d3p_dpvi_logreg_time_main_kernel": (C.c_int, [_V, _PM, _PH, _PS, _PB, _V, _V, _V, _SZ, C.c_int,
                                                   C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "d3p_selftest_wave_sums": (C.c_int, [_V, _V, _U32, _V]),
    "d3p_synth_logreg": (C.c_int, [_V, _U32, _U64, _U64, _I32, _V, _V]),
    "d3p_hbm_copy": (C.c_int, [_V, _V, _V, _U64, _I32]),
    "d3p_dpvi_leaves_begin": (C.c_int, [_V, _V, _I32, _V, _V, _U32, _V, _V, _V, _V]),
    "d3p_dpvi_leaves_finalize": (C.c_int, [_V, _PH, _V, _V, _V, C.POINTER(C.c_int32), _I32, _U32, C.c_float,
                                           _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    "d3p_px_eps_sites": (C.c_int, [_V, _V, _U32, _U32, _U32, C.POINTER(C.c_int32), _I32, _V]),
    "d3p_predict_draws": (C.c_int, [_V, _V, _U32, _I32, _I32, C.POINTER(PredictSite), _I32, _I32, _I32, _V, C.c_int64, _V]),
    "d3p_predict_logreg": (C.c_int, [_V, _V, _U64, _I32, _V, C.c_int64, _I32, _I32, _U32, _V, _V]),
    "d3p_predict_gauss": (C.c_int, [_V, _V, C.c_int64, _I32, _U64, _U32, _F, _V, _V]),
    "d3p_predict_vae_workspace": (_SZ, [_V, _U32, _U32]),
    "d3p_predict_vae": (C.c_int, [_V, _V, _V, _V, _U32, _V, _U32, _I32, _V, _V, _V, _V, _SZ]),
    # pointwise log-likelihoods over posterior draws (d3p_amd/infer_util.py): added symbols, ABI 9 unchanged
    "d3p_loglik_rows": (C.c_int, [_V, _PM, _V, _V, _U64, _V, C.c_int64, _I32, _I32, _U32, _V]),
    "d3p_loglik_lppd": (C.c_int, [_V, _PM, _V, _V, _U64, _V, C.c_int64, _I32, _I32, _U32, _V]),
    # WAIC over posterior draws, regression families and mixture model (d3p_amd/criteria.py): added symbols, ABI 9 unchanged
    "d3p_loglik_waic": (C.c_int, [_V, _PM, _V, _V, _U64, _V, C.c_int64, _I32, _I32, _U32, _U32, _V, _V]),
    "d3p_gmm_loglik_waic": (C.c_int, [_V, _V, _U64, _I32, _V, C.c_int64, _I32, _U32, _U32, _V, _V]),
    # PSIS-LOO per row of a draws x rows log-likelihood matrix (d3p_amd/criteria.py): added symbol, ABI 9 unchanged
    "d3p_psis_loo": (C.c_int, [_V, _V, C.c_int64, _U32, _U64, _V, _V, _V]),
    # per-draw float64 sums of the pointwise log-likelihood over a whole table (d3p_amd/diagnostics.py): added symbols, ABI 9 unchanged
    "d3p_loglik_draw_sums_workspace": (_SZ, [_U64, _U32]),
    "d3p_loglik_draw_sums": (C.c_int, [_V, _PM, _V, _V, _U64, _V, C.c_int64, _I32, _I32, _U32, _V, _V, _SZ]),
    # posterior predictive mean and variance over posterior draws (d3p_amd/prediction.py): added symbol, ABI 9 unchanged
    "d3p_predict_moments": (C.c_int, [_V, _PM, _V, _U64, _V, C.c_int64, _I32, _I32, _U32, _V, _V]),
    # predictive sampling of linear and Poisson regression (d3p_amd/predictive.py): added symbol, ABI 9 unchanged
    "d3p_predict_glm": (C.c_int, [_V, _PM, _V, _U64, _I32, _V, C.c_int64, _I32, _I32, _U32, _V, _V]),
    # predictive sampling and cluster assignment of the mixture model (d3p_amd/mixture.py): added symbols, ABI 9 unchanged
    "d3p_predict_gmm_draws": (C.c_int, [_V, _V, _U32, _I32, _I32, _I32, _I32, _V, _V, _F, _V, _V, _V, _V, _V]),
    "d3p_predict_gmm_obs": (C.c_int, [_V, _V, C.c_int64, _I32, _I32, _U64, _U32, _V, _V, _V]),
    "d3p_gmm_assign": (C.c_int, [_V, _V, _U64, _I32, _V, _V, _V, _I32, _V, _V]),
    # log predictive density and responsibilities of the mixture model over posterior draws (d3p_amd/mixture_density.py): added
    # symbols, ABI 9 unchanged
    "d3p_gmm_loglik_rows": (C.c_int, [_V, _V, _U64, _I32, _V, C.c_int64, _I32, _U32, _V]),
    "d3p_gmm_loglik_reduce": (C.c_int, [_V, _V, _U64, _I32, _V, C.c_int64, _I32, _U32, _V, _V]),
    # per-draw float64 sums of the mixture's pointwise log-likelihood over a whole table (d3p_amd/mixture_diagnostics.py): added symbols,
    # ABI 9 unchanged
    "d3p_gmm_loglik_draw_sums_workspace": (_SZ, [_U64, _I32, _I32, _U32]),
    "d3p_gmm_loglik_draw_sums": (C.c_int, [_V, _V, _U64, _I32, _V, C.c_int64, _I32, _U32, _V, _V, _SZ]),
    # log importance weights of the VAE's guide draws and per-column float64 statistics (d3p_amd/vae_density.py): added symbols, ABI 9
    # unchanged
    "d3p_vae_log_weights_workspace": (_SZ, [_V, _U32, _U32]),
    "d3p_vae_log_weights": (C.c_int, [_V, _V, _V, _V, _U32, _V, _U32, _I32, _U32, _V, _V, _V, _V, _SZ]),
    "d3p_vae_logw_rows": (C.c_int, [_V, _V, _V, _V, _V, _V, _U32, _U32, _I32, _I32, _V, _V]),
    "d3p_col_stats": (C.c_int, [_V, _V, C.c_int64, _U32, _U64, _V]),
    # per-column quantiles of a draws x cols matrix and the conditional mean's rows form (d3p_amd/intervals.py): added symbols, ABI 9 unchanged
    "d3p_col_quantiles": (C.c_int, [_V, _V, _I32, C.c_int64, _U32, _U64, _U32, C.POINTER(C.c_uint32), C.POINTER(C.c_double), _V, C.c_int64]),
    "d3p_col_quantiles_staged_max": (C.c_uint32, []),
    "d3p_predict_mean_rows": (C.c_int, [_V, _PM, _V, _U64, _V, C.c_int64, _I32, _I32, _U32, _V, C.c_int64]),
    # highest-density intervals per column of a draws x cols matrix, sorted in LDS (d3p_amd/intervals.py): added symbols, ABI 9 unchanged
    "d3p_col_hpdi": (C.c_int, [_V, _V, _I32, C.c_int64, _U32, _U64, _U32, C.POINTER(C.c_uint32), _V, C.c_int64]),
    "d3p_col_hpdi_max_n": (C.c_uint32, []),
    "d3p_col_hpdi_cols_per_group": (C.c_uint32, [_U32]),
    # CRPS and rank (PIT) counts per column of a draws x cols matrix against an observation (d3p_amd/scoring.py): added symbols, ABI 9 unchanged
    "d3p_col_crps": (C.c_int, [_V, _V, _I32, C.c_int64, _U32, _U64, _V, _V, C.c_int64, _V, C.c_int64]),
    "d3p_col_crps_max_n": (C.c_uint32, []),
    "d3p_col_crps_cols_per_group": (C.c_uint32, [_U32]),
    # per-example gradient norms without the rows and the profile of a vector of norms (d3p_amd/clipping.py): added symbols, ABI 9 unchanged
    "d3p_logreg_grad_norms_workspace": (_SZ, [_PM, _U32]),
    "d3p_logreg_grad_norms": (C.c_int, [_V, _PM, _V, _V, _V, _U32, _U32, _U32, _V, _V, _V, _V, _V, _SZ]),
    "d3p_norm_profile_workspace": (_SZ, [_U64]),
    "d3p_norm_profile": (C.c_int, [_V, _V, _U64, _U32, C.POINTER(C.c_float), _U32, C.POINTER(C.c_uint64), C.POINTER(C.c_double), _V, _V, _SZ]),
    # multi-particle ELBO (Trace_ELBO(num_particles=K)): added symbols, ABI 9 unchanged
    "d3p_logreg_px_grads_particles_workspace": (_SZ, [_PM, _U32, _U32]),
    "d3p_logreg_particles_max_latent": (C.c_int, [C.c_int]),
    "d3p_logreg_px_grads_particles": (C.c_int, [_V, _PM, _V, _V, _V, _V, _U32, _U32, _V, _V, _V, _V, _V, _V, _SZ]),
    "d3p_dpvi_logreg_local_sums_particles": (C.c_int, [_V, _PM, _PH, _PS, _PB, _V, _V, _V, _U32, _V, _V, _SZ]),
    "d3p_dpvi_logreg_run_particles_from": (C.c_int, [_V, _PM, _PH, _PS, _PS, _PB, _U32, _V, _V, _U32, _U32, _V, _V, _SZ]),
    "d3p_logreg_evaluate_particles_workspace": (_SZ, [_PM, _U32, _U32]),
    "d3p_logreg_evaluate_particles": (C.c_int, [_V, _PM, _V, _V, _V, _U32, _V, _U32, _V, _V, _SZ]),
    "d3p_logreg_evaluate_sites_particles": (C.c_int, [_V, _PM, _V, _V, _V, _U32, _V, C.POINTER(C.c_int32), _I32, _U32, _V, _V,
                                                      _SZ]),
    "d3p_px_eps_sites_particles": (C.c_int, [_V, _V, _U32, _U32, _U32, _U32, C.POINTER(C.c_int32), _I32, _V]),
    # stacking and Bayesian-bootstrap (pseudo-BMA+) model weights from pointwise elpd vectors (d3p_amd/model_weights.py): added symbols,
    # ABI 9 unchanged
    "d3p_stacking_workspace": (_SZ, [_U64, _U32]),
    "d3p_stacking_weights": (C.c_int, [_V, _V, C.c_int64, _U64, _U32, C.c_double, _U32, _V, _V, _V, _SZ]),
    "d3p_stacking_set_chunk": (C.c_int, [_I32]),
    "d3p_stacking_strip_rows": (C.c_uint32, []),
    "d3p_bb_pseudo_bma_workspace": (_SZ, [_U64, _U32, _U32]),
    "d3p_bb_pseudo_bma": (C.c_int, [_V, _V, _V, C.c_int64, _U64, _U32, _U32, _V, _V, _V, _SZ]),
    "d3p_bb_pseudo_bma_strip_rows": (C.c_uint32, []),
    # per-draw statistics of a replicated data set over its rows, from a matrix or fused with the outcome rules (d3p_amd/ppc.py): added
    # symbols, ABI 9 unchanged
    "d3p_rep_stats_workspace": (_SZ, [_U64, _U32]),
    "d3p_rep_stats": (C.c_int, [_V, _V, _I32, C.c_int64, _U32, _U64, C.c_double, _V, _V, _SZ]),
    "d3p_predict_stats": (C.c_int, [_V, _PM, _V, _U64, _I32, _V, C.c_int64, _I32, _I32, _U32, _V, C.c_double, _V, _V, _SZ]),
    # realized-discrepancy (chi-square) sums and the sums of the Bayesian R^2 per draw, fused with the outcome rules and the conditional
    # mean (d3p_amd/discrepancy.py): added symbols, ABI 9 unchanged
    "d3p_predict_discrepancy_workspace": (_SZ, [_U64, _U32]),
    "d3p_predict_discrepancy": (C.c_int, [_V, _PM, _V, _V, _U64, _I32, _V, C.c_int64, _I32, _I32, _U32, _V, C.c_double, _V, _V, _SZ]),
    # per-draw confusion counts fused with the outcome rule and the conditional mean, and the ROC histogram / reliability table of one
    # score vector (d3p_amd/classification.py): added symbols, ABI 9 unchanged
    "d3p_predict_confusion_set_strips": (C.c_int, [_I32]),
    "d3p_predict_confusion": (C.c_int, [_V, _PM, _V, _V, _U64, _I32, _V, C.c_int64, _I32, _I32, _U32, _V, C.POINTER(C.c_float), _I32, _V]),
    "d3p_binary_curve_workspace": (_SZ, []),
    "d3p_binary_curve": (C.c_int, [_V, _V, _V, _U64, _U32, _V, _V, _V, _V, _SZ]),
    # the energy score of (draws, rows, d) predictive draws against rows x d observations (d3p_amd/energy.py): added symbols, ABI 9 unchanged
    "d3p_energy_score": (C.c_int, [_V, _V, _I32, C.c_int64, C.c_int64, _U32, _U64, _U32, _V, C.c_int64, _V, C.c_int64]),
    "d3p_energy_score_max_n": (C.c_uint32, []),
    "d3p_energy_score_tile_draws": (C.c_uint32, []),
    "d3p_energy_score_chunk_cols": (C.c_uint32, []),
    "d3p_energy_score_rows_per_group": (C.c_uint32, [_I32]),
    "d3p_energy_score_form": (C.c_uint32, [_U32, _U64, _U32]),
    "d3p_energy_score_set_form": (C.c_int, [_I32]),
    # pair statistics of two tables: per-row distance sums, nearest row and its index (d3p_amd/fidelity.py): added symbols, ABI 9 unchanged
    "d3p_pair_stats": (C.c_int, [_V, _V, _V, _I32, C.c_int64, C.c_int64, _U32, _U32, _U32, _I32, _V, _V, _V, _V, _SZ]),
    "d3p_pair_stats_tile_rows": (C.c_uint32, []),
    "d3p_pair_stats_chunk_cols": (C.c_uint32, []),
    "d3p_pair_stats_segment_tiles": (C.c_uint32, []),
    "d3p_pair_stats_form": (C.c_uint32, [_U32, _U32, _U32]),
    "d3p_pair_stats_workspace": (_SZ, [_U32, _U32, _U32]),
    "d3p_pair_stats_set_form": (C.c_int, [_I32]),
    # binned one- and two-way marginal counts of a table (d3p_amd/marginals.py): added symbols, ABI 9 unchanged
    "d3p_marginals": (C.c_int, [_V, _V, _I32, C.c_int64, _U32, _U32, _U32, _V, _V, _V, _V, _V, _SZ]),
    "d3p_marginals_max_bins": (C.c_uint32, []),
    "d3p_marginals_strip_rows": (C.c_uint32, []),
    "d3p_marginals_pair_tile": (C.c_uint32, []),
    "d3p_marginals_code_rows": (C.c_uint32, []),
    "d3p_marginals_workspace": (_SZ, [_U32, _U32, _U32]),
    # label sums of the pooled pair distances for the energy distance's permutation test (d3p_amd/permutation.py): added symbols, ABI 9
    # unchanged
    "d3p_pair_label_sums": (C.c_int, [_V, _V, _I32, C.c_int64, _U32, _U32, _U32, _V, _V, _V, _V, _V, _V, _SZ]),
    "d3p_pair_label_sums_tile_rows": (C.c_uint32, []),
    "d3p_pair_label_sums_block_labellings": (C.c_uint32, []),
    "d3p_pair_label_sums_max_labellings": (C.c_uint32, []),
    "d3p_pair_label_sums_workspace": (_SZ, [_U32, _U32, _U32]),
}

_lib = None


def load():
    """dlopen libd3p_hip.so and attach signatures (no GPU required for this step)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise D3PError(
                f"{_SO} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  d3p_amd has no CPU fallback.")
        # torch bundles its own libamdhip64; import it first so that the loader binds this
        # library to the SAME HIP runtime instance (two runtimes in one process do not share a device)
        import torch  # noqa: F401
        # D3P_HIP_LIBRARY: a developer switch -- load another build of the library (diagnostic instantiations: tools/gemm_diag.sh)
        lib = C.CDLL(os.environ.get("D3P_HIP_LIBRARY") or _SO)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.d3p_abi_version() != 9:
            raise D3PError("libd3p_hip.so ABI version mismatch")
        _lib = lib
    return _lib


_device_checked = False


def require_device():
    """Fail loudly unless torch sees a ROCm device and the library can reach it."""
    global _device_checked
    if _device_checked:
        return
    import torch
    if not torch.cuda.is_available():
        raise D3PError("d3p_amd needs a ROCm GPU (MI355X / gfx950): torch.cuda.is_available() is "
                       "False and there is no CPU fallback.")
    if load().d3p_device_count() <= 0:
        raise D3PError("libd3p_hip.so sees no HIP device")
    _device_checked = True


def check(rc):
    if rc != 0:
        msg = load().d3p_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(msg)
        raise D3PError(f"libd3p_hip error {rc}: {msg}")


def stream_ptr():
    """The current torch stream of the current device as a raw hipStream_t (the fast accessor when this torch has it:
    torch.cuda.current_stream() costs ~9 us per call, which matters for per-step calls)."""
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return C.c_void_p(raw(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device address of a torch tensor (None -> NULL)."""
    if t is None:
        return C.c_void_p(0)
    return C.c_void_p(t.data_ptr())


_ABORT_KINDS = {1: "a bounded wait", 2: "exchange workgroup: the step's compute workgroups did not all arrive",
                3: "exchange workgroup: the row of a rank did not come (detail = that rank)",
                4: "compute workgroup: the previous step was not released (detail 1: by the exchange)",
                5: "key-chain workgroup: the previous link did not come", 6: "exchange kernel: the row of a rank did not come"}


def describe_abort(code: int) -> str:
    """Text of a run's abort code (d3p_logreg_kernel.h: kind | step << 8 | detail << 20); '' for 0."""
    code = int(code) & 0xffffffff
    if code == 0:
        return ""
    kind, step, detail = code & 0xff, (code >> 8) & 0xfff, (code >> 20) & 0xfff
    return f"{_ABORT_KINDS.get(kind, 'unknown wait')} [kind {kind}, step {step} of its launch, detail {detail}]"
