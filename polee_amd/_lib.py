"""ctypes binding of libpolee_hip.so (include/polee_hip.h).

The library is built in-tree by `__graft_entry__.build()` (or `make -C polee_amd/csrc`).
There is no CPU fallback: if the shared library is missing, importing the kernels fails
loudly, and without a GPU `Context()` raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# (POLEE_HIP_LIB: another build of the same library -- the toolchain gate test loads csrc/libpolee_hip_untuned.so)
LIB_PATH = os.environ.get("POLEE_HIP_LIB") or os.path.join(_HERE, "csrc", "libpolee_hip.so")

_lib = None

f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)
i32p = C.POINTER(C.c_int32)
i64p = C.POINTER(C.c_int64)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
u8p = C.POINTER(C.c_uint8)


class PoleeError(RuntimeError):
    """A libpolee_hip call failed; mirrors the reference's error()/@assert exceptions."""

    def __init__(self, status, message):
        super().__init__("polee_hip status %d: %s" % (status, message))
        self.status = status


class NonFiniteError(PoleeError, FloatingPointError):
    """POLEE_ERR_NONFINITE: the @assert isfinite(...) of the reference."""


class ViOpts(C.Structure):
    _fields_ = [("num_steps", C.c_int32), ("num_mc_samples", C.c_int32), ("use_efflen_jacobian", C.c_int32),
                ("gradonly", C.c_int32), ("seed", C.c_uint64), ("z0", f32p), ("y_eps", C.c_double),
                ("adam_initial_learning_rate", C.c_double), ("adam_learning_rate_decay", C.c_double),
                ("adam_min_learning_rate", C.c_double), ("adam_eps", C.c_double), ("adam_rv", C.c_double),
                ("adam_rm", C.c_double), ("max_mu_step", C.c_double), ("max_omega_step", C.c_double),
                ("max_alpha_step", C.c_double), ("profile", C.c_int32), ("deterministic", C.c_int32),
                ("gene_of", C.POINTER(C.c_int32))]


class ViStats(C.Structure):
    _fields_ = [("steps_done", C.c_int32), ("nonfinite_step", C.c_int32), ("loglik_kernel_ms_avg", C.c_double),
                ("loglik_kernel_launches", C.c_int64), ("last_elbo", C.c_double), ("last_lp_mean", C.c_double), ("loglik_pass_ms_avg", C.c_double)]


class AltViOpts(C.Structure):
    """polee_altvi_opts (include/polee_hip.h)"""
    _fields_ = [("method", C.c_int32), ("num_steps", C.c_int32), ("num_mc_samples", C.c_int32), ("gradonly", C.c_int32),
                ("refidx", C.c_int32), ("reserved", C.c_int32), ("seed", C.c_uint64), ("z0", f32p), ("eps", C.c_double),
                ("adam_initial_learning_rate", C.c_double), ("adam_learning_rate_decay", C.c_double),
                ("adam_min_learning_rate", C.c_double), ("adam_eps", C.c_double), ("adam_rv", C.c_double),
                ("adam_rm", C.c_double), ("max_step0", C.c_double), ("max_step1", C.c_double)]


class AltViStats(C.Structure):
    _fields_ = [("steps_done", C.c_int32), ("nonfinite_step", C.c_int32), ("last_elbo", C.c_double), ("last_lp_mean", C.c_double)]


class BiasTrainOpts(C.Structure):
    """polee_bias_train_opts (include/polee_hip.h)"""
    _fields_ = [("seed", C.c_uint64), ("host", C.c_int32), ("reserved", C.c_int32)]


class LoglikInfo(C.Structure):
    _fields_ = [("m", C.c_int64), ("n", C.c_int64), ("nnz", C.c_int64), ("num_slices", C.c_int64),
                ("num_tiles", C.c_int64), ("padded_nnz", C.c_int64), ("device_bytes", C.c_int64),
                ("stream_bytes", C.c_int64), ("num_empty_rows", C.c_int64), ("max_row_nnz", C.c_int32),
                ("max_tile_cols", C.c_int32), ("stream_rows", C.c_int64 * 8), ("stream_nnz", C.c_int64 * 8),
                ("stream_tiles", C.c_int64 * 8), ("stream_bytes_hbm", C.c_int64 * 8), ("dict_entries", C.c_int64)]


class PsellView(C.Structure):
    _fields_ = [("m", C.c_int64), ("n", C.c_int64), ("nnz", C.c_int64), ("num_slices", C.c_int64),
                ("num_tiles", C.c_int64), ("padded_nnz", C.c_int64), ("num_empty_rows", C.c_int64),
                ("data_bytes", C.c_int64), ("dict_len", C.c_int64), ("max_row_nnz", C.c_int32),
                ("max_tile_cols", C.c_int32), ("data", u8p), ("slice_off", u32p), ("tile_slice", u32p),
                ("tile_dict", u32p), ("dict", u32p), ("row_order", u32p), ("slice_ks", f32p), ("slice_flags", u8p),
                ("num_tiles_a", C.c_int64), ("num_tiles_a1", C.c_int64), ("num_tiles_a1m", C.c_int64), ("num_tiles_a2", C.c_int64), ("slice_w", u8p), ("num_tiles_s", C.c_int64),
                ("stream_rows", C.c_int64 * 8), ("stream_nnz", C.c_int64 * 8), ("stream_bytes", C.c_int64 * 8),
                ("csr_num_rows", C.c_int64), ("csr_rowptr", u32p), ("csr_col", u32p), ("csr_val", f32p), ("csr_rows", u32p),
                ("single_num_rows", C.c_int64), ("single_rows", u32p), ("single_cnt", f32p), ("single_logsum", C.c_double)]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "libpolee_hip.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C polee_amd/csrc`. There is no CPU fallback." % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.polee_last_error.restype = C.c_char_p
        L.polee_last_error.argtypes = [C.c_void_p]
        L.polee_version.restype = C.c_char_p
        L.polee_ctx_stream.restype = C.c_void_p
        L.polee_ctx_stream.argtypes = [C.c_void_p]
        L.polee_ptt_n.restype = C.c_int32
        L.polee_ptt_n.argtypes = [C.c_void_p]
        for name in ("polee_ctx_destroy", "polee_ptt_destroy", "polee_loglik_destroy", "polee_vi_destroy",
                     "polee_approx_destroy", "polee_debug_psell_free", "polee_comm_destroy", "polee_devx_destroy",
                     "polee_gibbs_destroy", "polee_em_destroy", "polee_altvi_destroy", "polee_bias_train_destroy",
                     "polee_regression_destroy", "polee_effects_destroy", "polee_sampler_destroy", "polee_classify_destroy",
                     "polee_tsne_destroy", "polee_forest_destroy", "polee_xbuild_destroy", "polee_splice_destroy"):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [C.c_void_p]
        L.polee_vi_default_opts.restype = None
        L.polee_altvi_default_opts.restype = None
        L.polee_altvi_default_opts.argtypes = [C.c_int32, C.POINTER(AltViOpts)]
        L.polee_altvi_create.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(AltViOpts), C.POINTER(C.c_void_p)]
        L.polee_altvi_run.argtypes = [C.c_void_p, C.c_int32]
        L.polee_altvi_sync.argtypes = [C.c_void_p]
        L.polee_altvi_get_params.argtypes = [C.c_void_p, f32p, f32p]
        L.polee_altvi_set_params.argtypes = [C.c_void_p, f32p, f32p]
        L.polee_altvi_get_stats.argtypes = [C.c_void_p, C.POINTER(AltViStats)]
        L.polee_altvi_get_trace.argtypes = [C.c_void_p, f64p, f64p]
        L.polee_altvi_export_noise.argtypes = [C.c_void_p, C.c_int32, f32p]
        L.polee_altvi_eval_gradients.argtypes = [C.c_void_p, f32p, f64p, f64p, f32p, f32p, f64p, f64p]
        L.polee_alt_sample.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, f32p, f32p, f32p, C.c_int32, C.c_int32,
                                       C.c_uint64, f32p, f32p]
        L.polee_ilr_coefficients.argtypes = [i32p, i32p, C.c_int64, f64p]
        # polee fit-tree (polee_amd/fit_tree.py)
        L.polee_kmer_sketch.argtypes = [C.c_void_p, C.c_int64, i64p, u8p, u64p]
        L.polee_kmer_sketch_host.argtypes = [C.c_int64, i64p, u8p, u64p]
        L.polee_kmer_tree_host.argtypes = [C.c_int64, u64p, i32p, i32p]
        L.polee_kmer_tree.argtypes = [C.c_void_p, C.c_int64, u64p, i32p, i32p]
        L.polee_fit_tree.argtypes = [C.c_void_p, C.c_int64, i64p, u8p, i32p, i32p]
        L.polee_debug_kmer_edges_count.argtypes = [C.c_void_p, C.c_int64, u64p, C.POINTER(C.c_int64)]
        L.polee_debug_kmer_edges_fill.argtypes = [C.c_void_p, C.c_int64, u64p, C.c_int64, u32p, u32p, u32p, u32p]
        L.polee_kmer_tree_rounds_host.argtypes = [C.c_int64, u64p, i32p, i32p, i64p]
        L.polee_kmer_tree_rounds.argtypes = [C.c_void_p, C.c_int64, u64p, i32p, i32p, i64p]
        L.polee_fit_tree_rounds.argtypes = [C.c_void_p, C.c_int64, i64p, u8p, i32p, i32p, i64p]
        L.polee_debug_kmer_round_select.argtypes = [C.c_void_p, C.c_int64, C.c_int64, u32p, u32p, u64p, u8p, i32p]
        # training of the bias model (polee_amd/bias.py)
        L.polee_bias_train_create.argtypes = [C.c_void_p, C.c_int32, i64p, u8p, C.c_int64, i32p, i64p, i32p, C.c_int64, i32p, i64p, i32p,
                                              C.POINTER(BiasTrainOpts), C.POINTER(C.c_void_p)]
        L.polee_bias_train_create_from_examples.argtypes = [C.c_void_p, C.c_int64, C.c_int64, u8p, u8p, f64p, C.POINTER(BiasTrainOpts),
                                                            C.POINTER(C.c_void_p)]
        L.polee_bias_train_run.argtypes = [C.c_void_p]
        L.polee_bias_train_get_model.argtypes = [C.c_void_p, i32p, i32p, f32p, f32p, f32p, f32p, f64p]
        L.polee_bias_train_get_examples.argtypes = [C.c_void_p, i64p, i64p, u64p, u64p, f64p, i64p]
        L.polee_bias_train_get_trace.argtypes = [C.c_void_p, C.c_int32, i32p, i32p, f64p]
        L.polee_bias_train_candidates.argtypes = [C.c_void_p, C.c_int32, i32p, f64p, f64p]
        # the fragment model from the alignment pairs (polee_amd/fragmodel.py)
        L.polee_fragmodel_estimate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, i64p, i64p, i64p]
        L.polee_read_assign.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, i64p, u8p, f32p, C.c_uint64, C.c_int32, C.c_int32,
                                        i32p, i64p, i32p, u8p]
        # splicing features from the exon structure (polee_amd/splicing.py)
        L.polee_splice_run.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.polee_splice_run_host.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
        L.polee_splice_sizes.argtypes = [C.c_void_p] + [i64p] * 6
        L.polee_splice_get.argtypes = [C.c_void_p] * 10
        _lib = L
    return _lib


def check(status, ctx=None):
    if status == 0:
        return
    msg = lib().polee_last_error(ctx).decode("utf-8", "replace")
    if status == 4:
        raise NonFiniteError(status, msg)
    raise PoleeError(status, msg)


class Handle:
    """Owner of a library handle self._h, released by the entry point named _destroy (declared in lib()).
    close() releases it now and may be called again; a class that holds more than its handle overrides close()
    and ends with super().close()."""
    _destroy = None
    _h = None

    def close(self):
        if self._h:
            getattr(lib(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def arr(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)
