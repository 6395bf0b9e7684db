"""ctypes binding of libcnf2hip.so (include/cnf2hip.h).

This is the Python host mirror used by tests and bench.py; the reference's own host side
is compiled C++, whose mirror is cnf2freq_amd/csrc/host (readers + CLI).  Everything that
computes goes through the C ABI; there is no CPU fallback: if the shared library is
missing or no HIP device is usable, calls raise.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CNF2HIP_LIB: another build of the same library (kernel A/B timing); still the HIP path, never a fallback
LIB_PATH = os.environ.get("CNF2HIP_LIB") or os.path.join(_HERE, "libcnf2hip.so")

OUT_DEVICE, NO_DOSAGE, RAW_DOSAGE, NO_TIES, FULL_SPILL, MERGE_MODES, ACC_DEVICE, ACC_KEEP, XPOSE, LOG_PATHS = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
ACC_TABLE = 1024
ACC_LANES = 2048
TIES_GENERAL = 4096
UPDATE_PLAIN = 8192
UPDATE_BOTH_FLOWS = 1 << 16       # both allele values' certainty flows (the bit-exact form of the fast update kernels)
UPDATE_ONE_SCOUT = 1 << 17        # the scouts (certainties', weights') in one pass instead of two (A/B)
UPDATE_LITERAL_FINISH = 1 << 19   # the set-aside flows one literal bisection step per round instead of the guided bisection (A/B)
DETERMINISTIC = 16384
TURN_VALU = 32768
FLUSH_TINY = 1 << 20              # cnf2_sweep: general kernel with adjustprobs' 1e-300 rule (the reference's behaviour to the letter)
ALL_STATES = 1 << 21              # windows of crosses of inbred lines through the fast kernel's ordinary instantiation (A/B, cross-check)
QTL_ADDITIVE = 1 << 22            # cnf2_qtl_scan / cnf2_sweep_qtl: the dominance column is always dropped
QTL_ORIGIN_DEVICE = 1 << 23       # cnf2_qtl_scan: the origin rows are a device pointer
QTL_REG_DEVICE = 1 << 28          # cnf2_qtl_scan_cols: the regressors are a device pointer
QTL_IMPRINT = 1 << 25             # cnf2_qtl_scanx: the design gets the imprinting effect i = o[1] - o[2]
QTL_STATE_DEVICE = 1 << 29        # cnf2_qtl_scan_imp: the sampled states are a device pointer
NO_UNIFORM_PACK = 1 << 26         # crosses of inbred lines: one window to a wave, not four windows of a chromosome (A/B, cross-check)
NO_UNIFORM_PACK8 = 1 << 27        # crosses of inbred lines: packed windows four to a wave only, not eight windows of a chromosome (A/B, cross-check)
NO_LINE_RECORDS = 1 << 24         # crosses of inbred lines: every window's emission terms from its own rows, not from the launch's line records (A/B, cross-check)
QTL_JOINT_DEVICE = 1 << 30        # cnf2_qtl_scan2_linked: the joint rows are a device pointer
STATIC_JOBS = 1 << 18            # wave w sweeps jobs w, w + waves, ... instead of taking jobs from the launch's counter (A/B)
MINFACTOR = float(np.float32(-1e15))
IGNORED = -1e30

# every symbol include/cnf2hip.h declares (checked by tests/test_capi_symbols.py)
SYMBOLS = [
    "cnf2_device_count", "cnf2_ctx_create", "cnf2_ctx_destroy", "cnf2_last_error", "cnf2_version",
    "cnf2_upload_map", "cnf2_upload_rows", "cnf2_update_rows", "cnf2_update_rows_device",
    "cnf2_upload_pedigree",
    "cnf2_window_info", "cnf2_sweep", "cnf2_sync", "cnf2_fwbw_store", "cnf2_locked_query",
    "cnf2_turn_scan", "cnf2_turn_scan_rows", "cnf2_state_posterior", "cnf2_haplos", "cnf2_infprobs", "cnf2_infprobs_rows", "cnf2_descendants", "cnf2_accumulate", "cnf2_sweep_accumulate", "cnf2_sweep_turn_scan", "cnf2_fixparents_scan", "cnf2_variances", "cnf2_variances_exact",
    "cnf2_snapshot_priors", "cnf2_update_pass", "cnf2_download_rows", "cnf2_download_accumulators", "cnf2_upload_accumulators", "cnf2_accumulator_ptrs", "cnf2_update_stats", "cnf2_update_stats_guided", "cnf2_addvariance", "cnf2_emission", "cnf2_emission_paths",
    "cnf2_selftest_lane_xor", "cnf2_last_kernel_ms", "cnf2_last_paths", "cnf2_workspace_bytes", "cnf2_reserve_accumulate", "cnf2_clock_probe", "cnf2_sweep_clock", "cnf2_stream",
    "cnf2_set_grid_reserve", "cnf2_set_batch_jobs", "cnf2_set_line_records", "cnf2_last_line_records", "cnf2_last_uniform_pack", "cnf2_last_uniform_pack8", "cnf2_last_plan_reused", "cnf2_last_plan_ms", "cnf2_window_table", "cnf2_update_pass_records", "cnf2_exchange_buffer", "cnf2_exchange_download", "cnf2_exchange_upload", "cnf2_exchange_read", "cnf2_exchange_write",
    "cnf2_packed_accumulator_doubles", "cnf2_packed_row_bytes", "cnf2_pack_accumulators", "cnf2_unpack_accumulators",
    "cnf2_pack_rows", "cnf2_unpack_rows",
    "cnf2_crossover_rows", "cnf2_sweep_crossovers", "cnf2_sweep_viterbi", "cnf2_sweep_sample",
    "cnf2_sweep_place", "cnf2_sweep_loo", "cnf2_loo_rows", "cnf2_sweep_origins", "cnf2_origin_rows",
    "cnf2_sweep_descent", "cnf2_descent_rows", "cnf2_qtl_scan_hap", "cnf2_qtl_scan_vc",
    "cnf2_linked_pairs", "cnf2_sweep_pairs", "cnf2_pair_rows", "cnf2_qtl_scan2_linked",
    "cnf2_qtl_scan", "cnf2_sweep_qtl", "cnf2_set_qtl_columns", "cnf2_qtl_scan2", "cnf2_set_qtl2_columns", "cnf2_qtl_scanx", "cnf2_set_qtlx_columns",
    "cnf2_qtl_scan_em", "cnf2_set_qtlem_columns", "cnf2_qtl_scan_binary", "cnf2_set_qtlbin_columns",
    "cnf2_qtl_scan_surv", "cnf2_set_qtlsurv_columns", "cnf2_set_qtlsurv_blocks",
    "cnf2_qtl_scan_var", "cnf2_set_qtlvar_columns",
    "cnf2_qtl_scan_cof", "cnf2_set_qtlcof_columns", "cnf2_qtl_kept_rows",
    "cnf2_kinship_sums", "cnf2_qtl_scan_fam", "cnf2_qtl_scan_cols", "cnf2_qtl_scan_boot", "cnf2_qtl_scan_mv", "cnf2_set_qtlmv_groups",
    "cnf2_qtl_scan_imp", "cnf2_set_qtlimp_columns",
]


class Cnf2Error(RuntimeError):
    pass


_lib = None


def hip_runtimes():
    """Paths of the HIP runtime libraries mapped into this process.  PyTorch's ROCm wheel carries its own libamdhip64.so
    (SONAME libamdhip64.so.7); libcnf2hip.so asks for libamdhip64.so.7.  If torch is imported FIRST the loader hands its
    copy to this library too (one runtime: device pointers, streams and RCCL buffers are interchangeable); the other way
    round torch loads a second copy next to /opt/rocm's and the two do not know each other's allocations.  Processes
    that use both import torch before the first cnf2freq_amd.capi.load()."""
    paths = set()
    try:
        for line in open("/proc/self/maps"):
            if "libamdhip64" in line:
                paths.add(line.split()[-1])
    except OSError:
        pass
    return sorted(paths)


def require_single_hip_runtime():
    r = hip_runtimes()
    if len(r) > 1:
        raise Cnf2Error("two HIP runtimes are loaded (%s): import torch before cnf2freq_amd loads libcnf2hip.so" % ", ".join(r))


def load():
    """Load libcnf2hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise Cnf2Error("libcnf2hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                            "or `make -C cnf2freq_amd/csrc`")
        L = C.CDLL(LIB_PATH)
        vp, i32 = C.c_void_p, C.c_int
        L.cnf2_device_count.restype = i32
        L.cnf2_ctx_create.argtypes = [i32, C.POINTER(vp)]
        L.cnf2_ctx_destroy.argtypes = [vp]
        L.cnf2_ctx_destroy.restype = None
        L.cnf2_last_error.argtypes = [vp]
        L.cnf2_last_error.restype = C.c_char_p
        L.cnf2_version.restype = C.c_char_p
        L.cnf2_upload_map.argtypes = [vp, vp, i32, vp, i32, vp]
        L.cnf2_upload_rows.argtypes = [vp, i32, vp, vp, vp]
        L.cnf2_update_rows.argtypes = [vp, i32, i32, vp, vp, vp]
        L.cnf2_update_rows_device.argtypes = [vp, i32, i32, vp, vp, vp]
        L.cnf2_upload_pedigree.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32]
        L.cnf2_window_info.argtypes = [vp, i32, vp]
        L.cnf2_sweep.argtypes = [vp, i32, i32, vp, vp, vp, C.c_uint32]
        L.cnf2_sync.argtypes = [vp]
        L.cnf2_fwbw_store.argtypes = [vp, i32, i32, vp, vp]
        L.cnf2_locked_query.argtypes = [vp, i32, i32, i32, vp]
        L.cnf2_turn_scan.argtypes = [vp, i32, i32, i32, vp]
        L.cnf2_turn_scan_rows.argtypes = [vp, i32, i32, vp]
        L.cnf2_state_posterior.argtypes = [vp, i32, i32, vp, C.c_uint32]
        L.cnf2_crossover_rows.argtypes = [vp, i32, i32, vp]
        L.cnf2_sweep_crossovers.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_sweep_viterbi.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_sweep_sample.argtypes = [vp, i32, i32, i32, C.c_uint64, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_sweep_place.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_sweep_loo.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_loo_rows.argtypes = [vp, i32, i32, vp]
        L.cnf2_sweep_origins.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_origin_rows.argtypes = [vp, i32, i32, vp]
        L.cnf2_sweep_descent.argtypes = [vp, i32, i32, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_descent_rows.argtypes = [vp, i32, i32, vp]
        L.cnf2_qtl_scan_hap.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_qtl_scan_vc.argtypes = [vp, i32, vp, vp, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_linked_pairs.argtypes = [vp, i32, vp, vp, vp]
        L.cnf2_sweep_pairs.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_pair_rows.argtypes = [vp, i32, i32, i32, vp, vp]
        L.cnf2_qtl_scan.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_sweep_qtl.argtypes = [vp, i32, i32, vp, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtl_columns.argtypes = [vp, i32]
        L.cnf2_qtl_scan2.argtypes = [vp, i32, vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_qtl_scan2_linked.argtypes = [vp, i32, vp, vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtl2_columns.argtypes = [vp, i32]
        L.cnf2_qtl_scanx.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtlx_columns.argtypes = [vp, i32]
        L.cnf2_qtl_scan_cof.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp,
                                        vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtlcof_columns.argtypes = [vp, i32]
        L.cnf2_qtl_kept_rows.argtypes = [vp, i32, i32, vp, vp]
        L.cnf2_kinship_sums.argtypes = [vp, i32, vp, i32, i32, vp, vp, C.c_uint32]
        L.cnf2_qtl_scan_fam.argtypes = [vp, i32, vp, i32, vp, vp, i32, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_qtl_scan_cols.argtypes = [vp, i32, i32, i32, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_qtl_scan_boot.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_qtl_scan_mv.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_qtl_scan_imp.argtypes = [vp, i32, i32, vp, i32, vp, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtlimp_columns.argtypes = [vp, i32]
        L.cnf2_set_qtlmv_groups.argtypes = [vp, i32]
        L.cnf2_qtl_scan_em.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, i32, C.c_double,
                                       vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtlem_columns.argtypes = [vp, i32]
        L.cnf2_qtl_scan_binary.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, vp, i32, C.c_double,
                                           vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtlbin_columns.argtypes = [vp, i32]
        L.cnf2_qtl_scan_surv.argtypes = [vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, vp, i32, C.c_double,
                                         vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtlsurv_columns.argtypes = [vp, i32]
        L.cnf2_set_qtlsurv_blocks.argtypes = [vp, i32]
        L.cnf2_qtl_scan_var.argtypes = [vp, i32, vp, i32, vp, vp, i32, vp, i32, i32, vp, i32, C.c_double,
                                        vp, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_set_qtlvar_columns.argtypes = [vp, i32]
        L.cnf2_haplos.argtypes = [vp, i32, i32, vp, C.c_uint32]
        L.cnf2_infprobs.argtypes = [vp, i32, i32, i32, vp, vp, C.c_uint32]
        L.cnf2_infprobs_rows.argtypes = [vp, i32, i32, vp, C.c_uint32]
        L.cnf2_addvariance.argtypes = [vp, i32, i32, vp]
        L.cnf2_descendants.argtypes = [vp, vp]
        L.cnf2_accumulate.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_sweep_accumulate.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint32]
        L.cnf2_reserve_accumulate.argtypes = [vp, i32, i32, C.c_uint32]
        L.cnf2_sweep_turn_scan.argtypes = [vp, i32, i32, vp, vp, C.c_uint32]
        L.cnf2_fixparents_scan.argtypes = [vp, vp, i32, vp]
        L.cnf2_variances.argtypes = [vp, vp, i32, i32, vp]
        L.cnf2_variances_exact.argtypes = [vp, vp, vp, i32, i32, vp]
        L.cnf2_snapshot_priors.argtypes = [vp, vp]
        L.cnf2_update_pass.argtypes = [vp, i32, vp, vp, vp, vp, vp, C.c_double, C.c_double, vp, C.c_uint32]
        L.cnf2_download_rows.argtypes = [vp, i32, i32, vp, vp, vp]
        L.cnf2_download_accumulators.argtypes = [vp, vp, vp, vp]
        L.cnf2_upload_accumulators.argtypes = [vp, vp, vp, vp]
        L.cnf2_accumulator_ptrs.argtypes = [vp, vp, vp, vp]
        L.cnf2_update_stats.argtypes = [vp, vp]
        L.cnf2_update_stats_guided.argtypes = [vp, vp]
        L.cnf2_emission.argtypes = [vp, i32, i32, vp]
        L.cnf2_emission_paths.argtypes = [vp, i32, i32, vp]
        L.cnf2_selftest_lane_xor.argtypes = [vp, vp]
        L.cnf2_last_kernel_ms.argtypes = [vp, vp, i32]
        L.cnf2_last_paths.argtypes = [vp, vp, i32]
        L.cnf2_workspace_bytes.argtypes = [vp]
        L.cnf2_workspace_bytes.restype = C.c_size_t
        L.cnf2_clock_probe.argtypes = [vp, vp]
        L.cnf2_sweep_clock.argtypes = [vp, vp]
        L.cnf2_set_grid_reserve.argtypes = [vp, i32]
        L.cnf2_set_batch_jobs.argtypes = [vp, i32]
        L.cnf2_set_line_records.argtypes = [vp, i32]
        L.cnf2_last_line_records.argtypes = [vp, vp]
        L.cnf2_last_uniform_pack.argtypes = [vp, vp]
        L.cnf2_last_uniform_pack8.argtypes = [vp, vp]
        L.cnf2_last_plan_reused.argtypes = [vp]
        L.cnf2_last_plan_ms.argtypes = [vp]
        L.cnf2_last_plan_ms.restype = C.c_float
        L.cnf2_window_table.argtypes = [vp, vp]
        L.cnf2_update_pass_records.argtypes = [vp, i32, vp, i32, vp, vp, C.c_double, C.c_double, vp, C.c_uint32]
        L.cnf2_exchange_buffer.argtypes = [vp, C.c_size_t, vp]
        L.cnf2_exchange_download.argtypes = [vp, vp, C.c_size_t]
        L.cnf2_exchange_upload.argtypes = [vp, vp, C.c_size_t]
        L.cnf2_exchange_read.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
        L.cnf2_exchange_write.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
        L.cnf2_packed_accumulator_doubles.argtypes = [vp]
        L.cnf2_packed_accumulator_doubles.restype = C.c_size_t
        L.cnf2_packed_row_bytes.argtypes = [vp]
        L.cnf2_packed_row_bytes.restype = C.c_size_t
        for f in (L.cnf2_pack_accumulators, L.cnf2_unpack_accumulators, L.cnf2_pack_rows, L.cnf2_unpack_rows):
            f.argtypes = [vp, vp, i32, vp]
        L.cnf2_stream.argtypes = [vp]
        L.cnf2_stream.restype = vp
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Context:
    """One GPU context (one per process/rank)."""

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.cnf2_ctx_create(device, C.byref(h))
        if rc != 0:
            raise Cnf2Error("cnf2_ctx_create: %s" % self.L.cnf2_last_error(None).decode())
        self.h = h
        self.device = device
        self.owned = True          # close() destroys the handle (False: Context.borrowed)
        self.n_markers = self.n_chrom = self.n_ind = self.n_rec = 0
        self.chromstarts = None

    @classmethod
    def borrowed(cls, handle, n_markers, chromstarts, n_ind, n_rec=0, device=0):
        """A Context over a cnf2_ctx handle that someone else owns and has uploaded to -- host.Run.context(), whose run read
        the files and holds the state of its rounds -- so that the analysis calls and cnf2freq_amd/qtl.py work on that state.
        The caller states what the owner uploaded (markers, chromstarts, analysed individuals) and the handle's device;
        close() leaves the handle alone, and the Context must not be used after its owner is closed."""
        self = cls.__new__(cls)
        self.L = load()
        self.h = C.c_void_p(handle)
        self.device = device
        self.owned = False
        self.n_markers, self.n_chrom, self.n_ind, self.n_rec = n_markers, len(chromstarts) - 1, n_ind, n_rec
        self.chromstarts = np.ascontiguousarray(chromstarts, np.int32)
        return self

    def close(self):
        if getattr(self, "h", None):
            if self.owned:
                self.L.cnf2_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise Cnf2Error("%s failed (%d): %s" % (what, rc, self.L.cnf2_last_error(self.h).decode()))

    # -- uploads ---------------------------------------------------------------
    def upload_map(self, pos, chromstarts, genrec=None):
        pos = np.ascontiguousarray(pos, np.float64)
        cs = np.ascontiguousarray(chromstarts, np.int32)
        g = None if genrec is None else np.ascontiguousarray(genrec, np.float64)
        self._chk(self.L.cnf2_upload_map(self.h, _p(pos), len(pos), _p(cs), len(cs) - 1,
                                         None if g is None else _p(g)), "cnf2_upload_map")
        self.n_markers, self.n_chrom, self.chromstarts = len(pos), len(cs) - 1, cs

    def upload_rows(self, allele, sure, hw):
        allele = np.ascontiguousarray(allele, np.uint8)
        sure = np.ascontiguousarray(sure, np.float64)
        hw = np.ascontiguousarray(hw, np.float64)
        assert allele.shape == sure.shape == hw.shape + (2,) and hw.shape[1] == self.n_markers
        self._chk(self.L.cnf2_upload_rows(self.h, hw.shape[0], _p(allele), _p(sure), _p(hw)), "cnf2_upload_rows")

    def alloc_blank_rows(self, n_rows):
        self._chk(self.L.cnf2_upload_rows(self.h, n_rows, None, None, None), "cnf2_upload_rows(blank)")

    def update_rows_device(self, row0, n, d_allele8, d_sure, d_hw):
        """Device pointers (ints): packed allele bytes [n][M], sure [n][M][2], hw [n][M]."""
        self._chk(self.L.cnf2_update_rows_device(self.h, row0, n, C.c_void_p(d_allele8), C.c_void_p(d_sure),
                                                 C.c_void_p(d_hw)), "cnf2_update_rows_device")

    def update_rows(self, row0, allele, sure, hw):
        allele = np.ascontiguousarray(allele, np.uint8)
        sure = np.ascontiguousarray(sure, np.float64)
        hw = np.ascontiguousarray(hw, np.float64)
        self._chk(self.L.cnf2_update_rows(self.h, row0, hw.shape[0], _p(allele), _p(sure), _p(hw)), "cnf2_update_rows")

    def upload_pedigree(self, par, empty, gen, row_of, dous):
        par = np.ascontiguousarray(par, np.int32)
        empty = np.ascontiguousarray(empty, np.uint8)
        gen = np.ascontiguousarray(gen, np.int32)
        row_of = np.ascontiguousarray(row_of, np.int32)
        dous = np.ascontiguousarray(dous, np.int32)
        self._chk(self.L.cnf2_upload_pedigree(self.h, len(par), _p(par), _p(empty), _p(gen), _p(row_of), _p(dous),
                                              len(dous)), "cnf2_upload_pedigree")
        self.n_ind = len(dous)
        self.n_rec = len(par)
        self.par, self.dous = par, dous        # (cnf2freq_amd.qtl.families reads the families off them)

    def upload(self, ped, dous=None):
        """Convenience: everything from a cnf2freq_amd.synth.Pedigree."""
        self.upload_map(ped.pos, ped.chromstarts)
        self.upload_rows(ped.allele, ped.sure, ped.hw)
        self.upload_pedigree(ped.par, ped.empty, ped.gen, ped.row_of, ped.dous if dous is None else dous)

    def upload_for_updates(self, ped, has_prior=None):
        """upload() in the form the update passes need: one genotype row per record (row 0 stays the blank row; updates
        write rows in place), and the rows remembered as priors (records that are not `empty` count as genotyped)."""
        a, s, h = ped.dense()
        R = ped.n_rec
        self.upload_map(ped.pos, ped.chromstarts)
        self.upload_rows(np.concatenate([a[:1] * 0, a]).astype(np.uint8), np.concatenate([s[:1] * 0, s]),
                         np.concatenate([h[:1] * 0 + 0.5, h]))
        self.upload_pedigree(ped.par, ped.empty, ped.gen, np.arange(1, R + 1, dtype=np.int32), ped.dous)
        self.snapshot_priors((1 - np.asarray(ped.empty)).astype(np.uint8) if has_prior is None else has_prior)

    def sweep_accumulate_keep(self, desc, ind_begin=0, ind_end=None, deterministic=False):
        """One haplotyping sweep whose accumulators stay in the context (for update_pass(..., acc=None),
        update_pass_records, pack_accumulators, download_accumulators)."""
        ind_end = self.n_ind if ind_end is None else ind_end
        desc = np.ascontiguousarray(desc, np.int32)
        self._chk(self.L.cnf2_sweep_accumulate(self.h, ind_begin, ind_end, _p(desc), None, None, None, None, None, None, None,
                                               DETERMINISTIC if deterministic else 0), "cnf2_sweep_accumulate")

    # -- the sweep -------------------------------------------------------------
    def sweep(self, ind_begin=0, ind_end=None, dosage=True, raw=False, ties=True, full_spill=False,
              merge_modes=False, xpose=False, log_paths=False, ties_general=False, static_jobs=False, flush_tiny=False, all_states=False,
              line_records=True, uniform_pack=True, uniform_pack8=True):
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        dos = np.zeros((n, self.n_markers, 3)) if dosage else None
        flags = ((0 if dosage else NO_DOSAGE) | (RAW_DOSAGE if raw else 0) | (0 if ties else NO_TIES)
                 | (FULL_SPILL if full_spill else 0) | (MERGE_MODES if merge_modes else 0) | (XPOSE if xpose else 0)
                 | (LOG_PATHS if log_paths else 0) | (TIES_GENERAL if ties_general else 0) | (STATIC_JOBS if static_jobs else 0) | (ALL_STATES if all_states else 0)
                 | (FLUSH_TINY if flush_tiny else 0) | (0 if line_records else NO_LINE_RECORDS)
                 | (0 if uniform_pack else NO_UNIFORM_PACK) | (0 if uniform_pack8 else NO_UNIFORM_PACK8))
        self._chk(self.L.cnf2_sweep(self.h, ind_begin, ind_end, _p(factors), _p(loglik),
                                    _p(dos) if dosage else None, flags), "cnf2_sweep")
        out = dict(factors=factors, loglik=loglik, dosage=dos)
        if log_paths:
            paths = np.zeros((n, self.n_chrom), np.int32)
            self._chk(self.L.cnf2_last_paths(self.h, _p(paths), paths.size), "cnf2_last_paths")
            out["paths"] = paths
        return out

    def sweep_device(self, ind_begin, ind_end, d_factors, d_loglik, d_dosage, flags=0):
        """Device-pointer form (ints or None); only enqueues on the context's stream."""
        self._chk(self.L.cnf2_sweep(self.h, ind_begin, ind_end, C.c_void_p(d_factors), C.c_void_p(d_loglik),
                                    C.c_void_p(d_dosage) if d_dosage else None, flags | OUT_DEVICE), "cnf2_sweep")

    def sync(self):
        self._chk(self.L.cnf2_sync(self.h), "cnf2_sync")

    def last_kernel_ms(self):
        ms = np.zeros(4, np.float32)
        self._chk(self.L.cnf2_last_kernel_ms(self.h, _p(ms), 4), "cnf2_last_kernel_ms")
        return float(ms[0])

    def set_grid_reserve(self, blocks):
        self._chk(self.L.cnf2_set_grid_reserve(self.h, blocks), "cnf2_set_grid_reserve")

    def set_line_records(self, lines):
        """Cap on the lines a sweep keeps records for (negative = none of its own, 0 = no records): cnf2_set_line_records."""
        self._chk(self.L.cnf2_set_line_records(self.h, lines), "cnf2_set_line_records")

    def last_line_records(self):
        """dict(lines, on_records, fallback, bytes) of the last sweep (cnf2_last_line_records)."""
        out = np.zeros(4, np.int32)
        self._chk(self.L.cnf2_last_line_records(self.h, _p(out)), "cnf2_last_line_records")
        return dict(lines=int(out[0]), on_records=int(out[1]), fallback=int(out[2]), bytes=int(out[3]))

    def last_uniform_pack(self):
        """dict(jobs, groups): the jobs of the last sweep that went four to a wave, and their groups (cnf2_last_uniform_pack)."""
        out = np.zeros(2, np.int32)
        self._chk(self.L.cnf2_last_uniform_pack(self.h, _p(out)), "cnf2_last_uniform_pack")
        return dict(jobs=int(out[0]), groups=int(out[1]))

    def last_uniform_pack8(self):
        """dict(eights, jobs): the pairs of groups of the last sweep that went eight to a wave, and their jobs (cnf2_last_uniform_pack8)."""
        out = np.zeros(2, np.int32)
        self._chk(self.L.cnf2_last_uniform_pack8(self.h, _p(out)), "cnf2_last_uniform_pack8")
        return dict(eights=int(out[0]), jobs=int(out[1]))

    def last_plan_reused(self):
        """True if the last sweep took the plan the context kept from the sweep before as it stood (cnf2_last_plan_reused)."""
        return bool(self.L.cnf2_last_plan_reused(self.h))

    def last_plan_ms(self):
        """Host milliseconds the last sweep spent before its first launch (cnf2_last_plan_ms)."""
        return float(self.L.cnf2_last_plan_ms(self.h))

    def set_batch_jobs(self, jobs):
        """Cap on the jobs per batch of sweep_accumulate / sweep_turn_scan (0 = what memory allows)."""
        self._chk(self.L.cnf2_set_batch_jobs(self.h, jobs), "cnf2_set_batch_jobs")

    def workspace_bytes(self):
        return int(self.L.cnf2_workspace_bytes(self.h))

    # -- parity hooks ------------------------------------------------------------
    def window_info(self, ind):
        out = np.zeros(17, np.int32)
        self._chk(self.L.cnf2_window_info(self.h, ind, _p(out)), "cnf2_window_info")
        return dict(shiftignore=int(out[0]), flag2ignore=int(out[1]), founder=int(out[2]),
                    slots=out[3:10].copy(), tie=out[10:17].copy())

    def fwbw_store(self, ind, chrom=0):
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        fw = np.zeros((8, mc, 3, 64))
        ff = np.zeros((8, mc, 3))
        self._chk(self.L.cnf2_fwbw_store(self.h, ind, chrom, _p(fw), _p(ff)), "cnf2_fwbw_store")
        return fw, ff

    def locked_query(self, ind, chrom, marker):
        v = np.zeros((8, 64, 128))
        self._chk(self.L.cnf2_locked_query(self.h, ind, chrom, marker, _p(v)), "cnf2_locked_query")
        return v

    def turn_scan(self, ind, chrom, marker):
        v = np.zeros((128, 8))
        self._chk(self.L.cnf2_turn_scan(self.h, ind, chrom, marker, _p(v)), "cnf2_turn_scan")
        return v

    def state_posterior(self, ind, chrom=0, ties=True):
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros((mc, 64))
        self._chk(self.L.cnf2_state_posterior(self.h, ind, chrom, _p(v), 0 if ties else NO_TIES), "cnf2_state_posterior")
        return v

    def crossover_rows(self, ind, chrom=0):
        """[mc][6] crossover posteriors of one individual and chromosome from the alpha/beta store, brute force (the
        cross-check of sweep_crossovers); column t = state bit t (include/cnf2hip.h: meiosis per column)."""
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros((mc, 6))
        self._chk(self.L.cnf2_crossover_rows(self.h, ind, chrom, _p(v)), "cnf2_crossover_rows")
        return v

    def sweep_crossovers(self, ind_begin=0, ind_end=None, rows=True, full_spill=False, ties_general=False,
                         static_jobs=False, all_states=False):
        """cnf2_sweep_crossovers: factors / loglik as sweep(), the per-individual crossover posteriors xo[n][M][6] (None
        with rows=False), their sum over the range xo_sum[M][6] and the contributing individuals per chromosome."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        xo = np.zeros((n, self.n_markers, 6)) if rows else None
        xs = np.zeros((self.n_markers, 6))
        cnt = np.zeros(self.n_chrom, np.int32)
        flags = ((FULL_SPILL if full_spill else 0) | (TIES_GENERAL if ties_general else 0)
                 | (STATIC_JOBS if static_jobs else 0) | (ALL_STATES if all_states else 0))
        self._chk(self.L.cnf2_sweep_crossovers(self.h, ind_begin, ind_end, _p(factors), _p(loglik),
                                               _p(xo) if rows else None, _p(xs), _p(cnt), flags),
                  "cnf2_sweep_crossovers")
        return dict(factors=factors, loglik=loglik, xo=xo, xo_sum=xs, n_contrib=cnt)

    def sweep_viterbi(self, ind_begin=0, ind_end=None, full_spill=False, ties_general=False, static_jobs=False, all_states=False,
                      line_records=True, uniform_pack=True, uniform_pack8=True):
        """cnf2_sweep_viterbi: factors / loglik as sweep(), logmax[n][C][8], the MAP state path state[n][M] (uint8, 0xFF
        where skipped), the MAP shift mode shift[n][C] (-1 where skipped) and path_logpost[n][C] = logmax[s*] - loglik,
        the log posterior probability of the decoded (mode, path) (NaN where skipped)."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        logmax = np.zeros((n, self.n_chrom, 8))
        state = np.zeros((n, self.n_markers), np.uint8)
        shift = np.zeros((n, self.n_chrom), np.int32)
        flags = ((FULL_SPILL if full_spill else 0) | (TIES_GENERAL if ties_general else 0)
                 | (STATIC_JOBS if static_jobs else 0) | (ALL_STATES if all_states else 0) | (0 if line_records else NO_LINE_RECORDS)
                 | (0 if uniform_pack else NO_UNIFORM_PACK) | (0 if uniform_pack8 else NO_UNIFORM_PACK8))
        self._chk(self.L.cnf2_sweep_viterbi(self.h, ind_begin, ind_end, _p(factors), _p(loglik), _p(logmax),
                                            _p(state), _p(shift), flags), "cnf2_sweep_viterbi")
        best = np.take_along_axis(logmax, np.maximum(shift, 0)[..., None], axis=2)[..., 0]
        path_logpost = np.where(shift >= 0, best - loglik, np.nan)
        return dict(factors=factors, loglik=loglik, logmax=logmax, state=state, shift=shift, path_logpost=path_logpost)

    def sweep_sample(self, ind_begin=0, ind_end=None, draws=1, seed=0, full_spill=False, ties_general=False,
                     static_jobs=False, all_states=False):
        """cnf2_sweep_sample: factors / loglik as sweep(), and `draws` (mode, path) draws from the posterior per individual
        and chromosome: state[n][K][M] (uint8, 0xFF where skipped), shift[n][K][C] (the drawn mode, -1 where skipped) and
        logp[n][K][C] = log P(mode, path | data) (NaN where skipped).  Draw k depends on (seed, individual, k) only."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        state = np.zeros((n, draws, self.n_markers), np.uint8)
        shift = np.zeros((n, draws, self.n_chrom), np.int32)
        logp = np.zeros((n, draws, self.n_chrom))
        flags = ((FULL_SPILL if full_spill else 0) | (TIES_GENERAL if ties_general else 0)
                 | (STATIC_JOBS if static_jobs else 0) | (ALL_STATES if all_states else 0))
        self._chk(self.L.cnf2_sweep_sample(self.h, ind_begin, ind_end, draws, int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           _p(factors), _p(loglik), _p(state), _p(shift), _p(logp), flags),
                  "cnf2_sweep_sample")
        logp = np.where(shift >= 0, logp, np.nan)
        return dict(factors=factors, loglik=loglik, state=state, shift=shift, logp=logp)

    def _candidate_rows(self, cand_allele, cand_sure, cand_hw):
        a = np.ascontiguousarray(cand_allele, np.uint8)
        s = np.ascontiguousarray(cand_sure, np.float64)
        h = None if cand_hw is None else np.ascontiguousarray(cand_hw, np.float64)
        assert a.ndim == 3 and a.shape[2] == 2 and a.shape == s.shape and (h is None or h.shape == a.shape[:2])
        return a, s, h

    def sweep_place(self, cand_allele, cand_sure, cand_hw=None, ind_begin=0, ind_end=None, per_individual=False,
                    full_spill=False, ties_general=False, static_jobs=False, all_states=False):
        """cnf2_sweep_place: where Q unmapped markers go.  cand_allele / cand_sure [n_rows][Q][2] and cand_hw [n_rows][Q]
        (None = 0.5) are the candidates' rows in the row index space of upload_rows.  Returns factors / loglik as sweep(),
        place_sum[Q][M] (the growth of the range's log-likelihood with candidate q laid at marker m, over the individuals
        that are neither skipped nor impossible there), n_zero[Q][M] (the impossible ones), null[Q] (the unlinked
        baseline), n_contrib[C], and with per_individual=True place[n][Q][M] (MINFACTOR where impossible, IGNORED where
        skipped), else None.  placement.best_positions reads the profile."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        a, s, h = self._candidate_rows(cand_allele, cand_sure, cand_hw)
        Q = a.shape[1]
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        place = np.zeros((n, Q, self.n_markers)) if per_individual else None
        psum = np.zeros((Q, self.n_markers))
        nz = np.zeros((Q, self.n_markers), np.int32)
        null = np.zeros(Q)
        cnt = np.zeros(self.n_chrom, np.int32)
        flags = ((FULL_SPILL if full_spill else 0) | (TIES_GENERAL if ties_general else 0)
                 | (STATIC_JOBS if static_jobs else 0) | (ALL_STATES if all_states else 0))
        self._chk(self.L.cnf2_sweep_place(self.h, ind_begin, ind_end, Q, _p(a), _p(s), None if h is None else _p(h),
                                          _p(factors), _p(loglik), _p(place) if per_individual else None, _p(psum),
                                          _p(nz), _p(null), _p(cnt), flags), "cnf2_sweep_place")
        return dict(factors=factors, loglik=loglik, place=place, place_sum=psum, n_zero=nz, null=null, n_contrib=cnt)

    def sweep_place_device(self, cand_allele, cand_sure, cand_hw, ind_begin, ind_end, d_factors, d_loglik, d_place,
                           d_place_sum, d_n_zero, d_null, d_n_contrib, flags=0):
        """Device-pointer form (ints; d_place may be None); the candidate rows stay host arrays."""
        a, s, h = self._candidate_rows(cand_allele, cand_sure, cand_hw)
        self._chk(self.L.cnf2_sweep_place(self.h, ind_begin, ind_end, a.shape[1], _p(a), _p(s), None if h is None else _p(h),
                                          C.c_void_p(d_factors), C.c_void_p(d_loglik),
                                          C.c_void_p(d_place) if d_place else None, C.c_void_p(d_place_sum),
                                          C.c_void_p(d_n_zero), C.c_void_p(d_null), C.c_void_p(d_n_contrib),
                                          flags | OUT_DEVICE), "cnf2_sweep_place")

    def loo_rows(self, ind, chrom=0):
        """[mc][2] = (loo, unlinked) of one individual and chromosome from the alpha/beta store, brute force (the
        cross-check of sweep_loo); IGNORED where the individual is skipped."""
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros((mc, 2))
        self._chk(self.L.cnf2_loo_rows(self.h, ind, chrom, _p(v)), "cnf2_loo_rows")
        return v

    def sweep_loo(self, ind_begin=0, ind_end=None, rows=True, full_spill=False, ties_general=False, static_jobs=False):
        """cnf2_sweep_loo: factors / loglik as sweep(); loo[n][M], the cost in nats of the data at marker m given the
        individual's data at every other marker of the chromosome, and unlinked[n][M], the cost of the same data with
        the marker off the map (both IGNORED where skipped; None with rows=False); their sums over the range's
        individuals loo_sum[M] / unlinked_sum[M] and the contributing individuals per chromosome.  qc.marker_report and
        qc.flag_genotypes read them."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        loo = np.zeros((n, self.n_markers)) if rows else None
        unl = np.zeros((n, self.n_markers)) if rows else None
        ls = np.zeros(self.n_markers)
        us = np.zeros(self.n_markers)
        cnt = np.zeros(self.n_chrom, np.int32)
        flags = ((FULL_SPILL if full_spill else 0) | (TIES_GENERAL if ties_general else 0)
                 | (STATIC_JOBS if static_jobs else 0))
        self._chk(self.L.cnf2_sweep_loo(self.h, ind_begin, ind_end, _p(factors), _p(loglik), _p(loo) if rows else None,
                                        _p(unl) if rows else None, _p(ls), _p(us), _p(cnt), flags), "cnf2_sweep_loo")
        return dict(factors=factors, loglik=loglik, loo=loo, unlinked=unl, loo_sum=ls, unlinked_sum=us, n_contrib=cnt)

    def sweep_loo_device(self, ind_begin, ind_end, d_factors, d_loglik, d_loo, d_unlinked, d_loo_sum, d_unlinked_sum,
                         d_n_contrib, flags=0):
        """Device-pointer form (ints; d_loo / d_unlinked may be None: the rows then stay in the context)."""
        self._chk(self.L.cnf2_sweep_loo(self.h, ind_begin, ind_end, C.c_void_p(d_factors), C.c_void_p(d_loglik),
                                        C.c_void_p(d_loo) if d_loo else None,
                                        C.c_void_p(d_unlinked) if d_unlinked else None, C.c_void_p(d_loo_sum),
                                        C.c_void_p(d_unlinked_sum), C.c_void_p(d_n_contrib), flags | OUT_DEVICE),
                  "cnf2_sweep_loo")

    def origin_rows(self, ind, chrom=0):
        """[mc][10] = origin[4], bits[6] of one individual and chromosome from the alpha/beta store, brute force (the
        cross-check of sweep_origins); zeros where the individual is skipped."""
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros((mc, 10))
        self._chk(self.L.cnf2_origin_rows(self.h, ind, chrom, _p(v)), "cnf2_origin_rows")
        return v

    def sweep_origins(self, ind_begin=0, ind_end=None, rows=True, full_spill=False, ties_general=False, static_jobs=False,
                      all_states=False):
        """cnf2_sweep_origins: factors / loglik as sweep(); origin[n][M][4], the probabilities that the alleles from the
        first and the second parent descend from those parents' (first, first), (second, first), (first, second) and
        (second, second) parent -- AA, BA, AB, BB by side in an F2 whose F1s list line A first -- and bits[n][M][6],
        P(meiosis bit t = 1) (both all zero where skipped; None with rows=False); origin_sum[M][4], their sum over the
        range's individuals, and the contributing individuals per chromosome.  The frame is absolute (include/cnf2hip.h).
        cnf2freq_amd/origins.py reads them.  all_states (CNF2_ALL_STATES) is accepted and changes nothing."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        origin = np.zeros((n, self.n_markers, 4)) if rows else None
        bits = np.zeros((n, self.n_markers, 6)) if rows else None
        osum = np.zeros((self.n_markers, 4))
        cnt = np.zeros(self.n_chrom, np.int32)
        flags = ((FULL_SPILL if full_spill else 0) | (TIES_GENERAL if ties_general else 0)
                 | (STATIC_JOBS if static_jobs else 0) | (ALL_STATES if all_states else 0))
        self._chk(self.L.cnf2_sweep_origins(self.h, ind_begin, ind_end, _p(factors), _p(loglik),
                                            _p(origin) if rows else None, _p(bits) if rows else None, _p(osum), _p(cnt),
                                            flags), "cnf2_sweep_origins")
        return dict(factors=factors, loglik=loglik, origin=origin, bits=bits, origin_sum=osum, n_contrib=cnt)

    def sweep_origins_device(self, ind_begin, ind_end, d_factors, d_loglik, d_origin, d_bits, d_origin_sum, d_n_contrib,
                             flags=0):
        """Device-pointer form (ints; d_origin / d_bits may be None: the rows then stay in the context)."""
        self._chk(self.L.cnf2_sweep_origins(self.h, ind_begin, ind_end, C.c_void_p(d_factors), C.c_void_p(d_loglik),
                                            C.c_void_p(d_origin) if d_origin else None,
                                            C.c_void_p(d_bits) if d_bits else None, C.c_void_p(d_origin_sum),
                                            C.c_void_p(d_n_contrib), flags | OUT_DEVICE), "cnf2_sweep_origins")

    # -- descent rows ------------------------------------------------------------
    def descent_rows(self, ind, chrom=0):
        """[mc][8], the descent row of one individual and chromosome from the alpha/beta store, brute force (the cross-check
        of sweep_descent); zeros where the individual is skipped."""
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros((mc, 8))
        self._chk(self.L.cnf2_descent_rows(self.h, ind, chrom, _p(v)), "cnf2_descent_rows")
        return v

    def sweep_descent(self, ind_begin=0, ind_end=None, rows=True, full_spill=False, ties_general=False, static_jobs=False):
        """cnf2_sweep_descent: factors / loglik as sweep(); descent[n][M][8], per side (0..3 the first parent's, 4..7 the
        second parent's) the probabilities of the classes 2 w + b -- the allele from that parent descends from the parent's
        par[.][w], strand b of that grandparent, the strand labelled by the grandparent's own record (allele order and hw;
        include/cnf2hip.h).  All zero where skipped; None with rows=False.  n_contrib: the contributing individuals per
        chromosome.  cnf2freq_amd/origins.py reads them (DESCENT_MASK, descent_columns, descent_calls)."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        descent = np.zeros((n, self.n_markers, 8)) if rows else None
        cnt = np.zeros(self.n_chrom, np.int32)
        flags = ((FULL_SPILL if full_spill else 0) | (TIES_GENERAL if ties_general else 0)
                 | (STATIC_JOBS if static_jobs else 0))
        self._chk(self.L.cnf2_sweep_descent(self.h, ind_begin, ind_end, _p(factors), _p(loglik),
                                            _p(descent) if rows else None, _p(cnt), flags), "cnf2_sweep_descent")
        return dict(factors=factors, loglik=loglik, descent=descent, n_contrib=cnt)

    def sweep_descent_device(self, ind_begin, ind_end, d_factors, d_loglik, d_descent, d_n_contrib, flags=0):
        """Device-pointer form (ints; d_descent may be None: the rows then stay in the context)."""
        self._chk(self.L.cnf2_sweep_descent(self.h, ind_begin, ind_end, C.c_void_p(d_factors), C.c_void_p(d_loglik),
                                            C.c_void_p(d_descent) if d_descent else None, C.c_void_p(d_n_contrib),
                                            flags | OUT_DEVICE), "cnf2_sweep_descent")

    # -- pair posteriors ---------------------------------------------------------
    def linked_pairs(self, sel):
        """cnf2_linked_pairs: pairs[n_pairs][2] (int32), the pairs j < k of indices into sel whose markers share a
        chromosome, in the order of sweep_pairs' rows (ascending j, then ascending k)."""
        sel = np.ascontiguousarray(sel, np.int32)
        cnt = np.zeros(1, np.int32)
        self._chk(self.L.cnf2_linked_pairs(self.h, len(sel), _p(sel), None, _p(cnt)), "cnf2_linked_pairs")
        pairs = np.zeros((int(cnt[0]), 2), np.int32)
        if len(pairs):
            self._chk(self.L.cnf2_linked_pairs(self.h, len(sel), _p(sel), _p(pairs), _p(cnt)), "cnf2_linked_pairs")
        return pairs

    def pair_rows(self, ind, chrom, sel):
        """[S (S - 1) / 2][16] the rows of sweep_pairs for one individual and the S markers of sel on one chromosome, from
        the alpha/beta store by brute force (the cross-check of sweep_pairs); zeros where the individual is skipped."""
        sel = np.ascontiguousarray(sel, np.int32)
        S = int(((sel >= self.chromstarts[chrom]) & (sel < self.chromstarts[chrom + 1])).sum())
        v = np.zeros((S * (S - 1) // 2, 16))
        self._chk(self.L.cnf2_pair_rows(self.h, ind, chrom, len(sel), _p(sel), _p(v)), "cnf2_pair_rows")
        return v

    def sweep_pairs(self, sel, ind_begin=0, ind_end=None, rows=True, ties_general=False, static_jobs=False):
        """cnf2_sweep_pairs: factors / loglik as sweep(); joint[n][n_pairs][16], for every pair of linked_pairs(sel) the joint
        distribution of the origin classes (u at the first, v at the second locus, cell 4 u + v; the classes and the frame
        are sweep_origins'; all zero where skipped; None with rows=False); joint_sum[n_pairs][16], their sum over the
        range's individuals, and the contributing individuals per chromosome.  cnf2freq_amd/origins.py reads them."""
        sel = np.ascontiguousarray(sel, np.int32)
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        NP = len(self.linked_pairs(sel))
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        joint = np.zeros((n, NP, 16)) if rows else None
        jsum = np.zeros((NP, 16))
        cnt = np.zeros(self.n_chrom, np.int32)
        flags = (TIES_GENERAL if ties_general else 0) | (STATIC_JOBS if static_jobs else 0)
        self._chk(self.L.cnf2_sweep_pairs(self.h, ind_begin, ind_end, len(sel), _p(sel), _p(factors), _p(loglik),
                                          _p(joint) if rows else None, _p(jsum), _p(cnt), flags), "cnf2_sweep_pairs")
        return dict(factors=factors, loglik=loglik, joint=joint, joint_sum=jsum, n_contrib=cnt)

    def sweep_pairs_device(self, ind_begin, ind_end, sel, d_factors, d_loglik, d_joint, d_joint_sum, d_n_contrib, flags=0):
        """Device-pointer form (ints; d_joint may be None: the rows then stay in the context)."""
        sel = np.ascontiguousarray(sel, np.int32)
        self._chk(self.L.cnf2_sweep_pairs(self.h, ind_begin, ind_end, len(sel), _p(sel), C.c_void_p(d_factors),
                                          C.c_void_p(d_loglik), C.c_void_p(d_joint) if d_joint else None,
                                          C.c_void_p(d_joint_sum), C.c_void_p(d_n_contrib), flags | OUT_DEVICE),
                  "cnf2_sweep_pairs")

    # -- QTL scan ----------------------------------------------------------------
    def set_qtl_columns(self, cap):
        """Cap on the phenotype columns per tile of qtl_scan / sweep_qtl (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtl_columns(self.h, cap), "cnf2_set_qtl_columns")

    @staticmethod
    def _qtl_inputs(n, pheno, cov, use, perm):
        """the phenotype side of a scan as contiguous arrays: (pheno[n][T], cov[n][K] or None, use[n] or None, perm[P][n] or None)"""
        pheno = np.ascontiguousarray(pheno, np.float64)
        if pheno.ndim == 1:
            pheno = pheno[:, None]
        if pheno.ndim != 2 or pheno.shape[0] != n:
            raise ValueError("pheno must be [n][T] with n = %d" % n)
        if cov is not None:
            cov = np.ascontiguousarray(cov, np.float64)
            cov = cov[:, None] if cov.ndim == 1 else cov
            if cov.ndim != 2 or cov.shape[0] != n:
                raise ValueError("cov must be [n][K]")
            if cov.shape[1] == 0:
                cov = None
        if use is not None:
            use = np.ascontiguousarray(np.asarray(use) != 0, np.uint8)
            if use.shape != (n,):
                raise ValueError("use must be [n]")
        if perm is not None:
            perm = np.ascontiguousarray(perm, np.int32)
            perm = perm[None, :] if perm.ndim == 1 else perm
            if perm.ndim != 2 or perm.shape[1] != n:
                raise ValueError("perm must be [P][n]")
            if perm.shape[0] == 0:
                perm = None
        return pheno, cov, use, perm

    @staticmethod
    def _n_effects(flags):
        """the effects a marker is fitted with: a, d unless QTL_ADDITIVE, i with QTL_IMPRINT"""
        return 1 + (0 if flags & QTL_ADDITIVE else 1) + (1 if flags & QTL_IMPRINT else 0)

    @staticmethod
    def _fit_flags(flags, additive, imprint):
        return flags | (QTL_ADDITIVE if additive else 0) | (QTL_IMPRINT if imprint else 0)

    def _origin_rows(self, origin):
        """origin as a contiguous float64 array [n][M][4], or ValueError"""
        origin = np.ascontiguousarray(origin, np.float64)
        if origin.ndim != 3 or origin.shape[1:] != (self.n_markers, 4):
            raise ValueError("origin must be [n][%d][4]" % self.n_markers)
        return origin

    def _qtl_outputs(self, T, P):
        M, Cn = self.n_markers, self.n_chrom
        return dict(lod=np.zeros((T, M)), coef=np.zeros((T, M, 2)), rank=np.zeros(M, np.int32), rss0=np.zeros((T, Cn)),
                    n_used=np.zeros(Cn, np.int32), perm_max=np.zeros((P, T, Cn)) if P else None)

    def _qtl_call(self, n, origin_ptr, pheno, cov, use, perm, flags, out=None):
        """cnf2_qtl_scan with host outputs (out = None: new arrays) on the rows behind origin_ptr"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        o = self._qtl_outputs(T, P) if out is None else out
        opt = lambda a: None if a is None else _p(a)
        self._chk(self.L.cnf2_qtl_scan(self.h, n, origin_ptr, T, _p(pheno), opt(use), K, opt(cov), P, opt(perm), _p(o["lod"]),
                                       _p(o["coef"]), _p(o["rank"]), _p(o["rss0"]), _p(o["n_used"]), opt(o["perm_max"]),
                                       flags), "cnf2_qtl_scan")
        return o

    def qtl_scan(self, origin, pheno, cov=None, use=None, perm=None, additive=False):
        """cnf2_qtl_scan on host rows origin[n][M][4] (what sweep_origins returns): Haley-Knott regression of pheno[n][T] on
        the rows at every marker, with fixed-effect covariates cov[n][K], the individuals of use[n] and the permutations
        perm[P][n].  A dict: lod[T][M], coef[T][M][2] (additive and dominance effect; NaN for a dropped column), rank[M],
        rss0[T][C], n_used[C], perm_max[P][T][C] (None without permutations).  The model: include/cnf2hip.h;
        cnf2freq_amd/qtl.py reads the results."""
        origin = self._origin_rows(origin)
        return self._qtl_call(origin.shape[0], _p(origin), pheno, cov, use, perm, QTL_ADDITIVE if additive else 0)

    def qtl_scan_device(self, n, d_origin, pheno, cov=None, use=None, perm=None, additive=False):
        """The same on device rows (d_origin: an int, the pointer of n x M x 4 doubles aligned to 16 bytes, e.g. the tensor a
        sweep_origins_device call filled); they are read in place.  Phenotypes and outputs are host arrays.  d_origin None:
        the rows this context's last sweep_qtl left in it (n that call's; Cnf2Error once anything has been uploaded or
        another call has used the buffer since)."""
        return self._qtl_call(n, C.c_void_p(d_origin), pheno, cov, use, perm,
                              QTL_ORIGIN_DEVICE | (QTL_ADDITIVE if additive else 0))

    def sweep_qtl(self, pheno, cov=None, use=None, perm=None, additive=False, ind_begin=0, ind_end=None, full_spill=False,
                  ties_general=False, static_jobs=False):
        """cnf2_sweep_qtl: the origin sweep of the range with the rows in the context, then the scan on them.  The dict of
        qtl_scan plus factors / loglik as sweep()."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        o = self._qtl_outputs(T, P)
        o["factors"] = np.zeros((n, self.n_chrom, 8))
        o["loglik"] = np.zeros((n, self.n_chrom))
        flags = ((FULL_SPILL if full_spill else 0) | (TIES_GENERAL if ties_general else 0)
                 | (STATIC_JOBS if static_jobs else 0) | (QTL_ADDITIVE if additive else 0))
        opt = lambda a: None if a is None else _p(a)
        self._chk(self.L.cnf2_sweep_qtl(self.h, ind_begin, ind_end, _p(o["factors"]), _p(o["loglik"]), T, _p(pheno), opt(use),
                                        K, opt(cov), P, opt(perm), _p(o["lod"]), _p(o["coef"]), _p(o["rank"]), _p(o["rss0"]),
                                        _p(o["n_used"]), opt(o["perm_max"]), flags), "cnf2_sweep_qtl")
        return o

    def sweep_qtl_device(self, ind_begin, ind_end, d_factors, d_loglik, pheno, cov, use, perm, d_lod, d_coef, d_rank, d_rss0,
                         d_n_used, d_perm_max, flags=0):
        """Device-pointer form (ints; d_perm_max None without permutations); phenotypes stay host arrays."""
        pheno, cov, use, perm = self._qtl_inputs(ind_end - ind_begin, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        opt = lambda a: None if a is None else _p(a)
        self._chk(self.L.cnf2_sweep_qtl(self.h, ind_begin, ind_end, C.c_void_p(d_factors), C.c_void_p(d_loglik), T, _p(pheno),
                                        opt(use), K, opt(cov), P, opt(perm), C.c_void_p(d_lod), C.c_void_p(d_coef),
                                        C.c_void_p(d_rank), C.c_void_p(d_rss0), C.c_void_p(d_n_used),
                                        C.c_void_p(d_perm_max) if d_perm_max else None, flags | OUT_DEVICE), "cnf2_sweep_qtl")

    # -- within-family scan --------------------------------------------------------
    QTLFAM_KEYS = ("lod", "df", "slope", "rss0", "n_used", "n_cells", "perm_max")

    def _qtlfam_call(self, n, origin_ptr, side, grp, cell, n_fam, pheno, cov, use, perm, slopes, flags, out=None):
        """cnf2_qtl_scan_fam with host outputs (out = None: new arrays) on the rows behind origin_ptr"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        grp = np.ascontiguousarray(grp, np.int32)
        cell = None if cell is None else np.ascontiguousarray(cell, np.int32)
        if grp.shape != (n,) or (cell is not None and cell.shape != (n,)):
            raise ValueError("grp and cell must be [n]")
        M, Cn, F = self.n_markers, self.n_chrom, int(n_fam)
        o = out
        if o is None:
            o = dict(lod=np.zeros((T, M)), df=np.zeros(M, np.int32), slope=np.zeros((T, M, max(F, 0))) if slopes else None,
                     rss0=np.zeros((T, Cn)), n_used=np.zeros(Cn, np.int32), n_cells=np.zeros(Cn, np.int32),
                     perm_max=np.zeros((P, T, Cn)) if P else None)
        opt = lambda a: None if a is None else _p(a)
        self._chk(self.L.cnf2_qtl_scan_fam(self.h, n, origin_ptr, int(side), _p(grp), opt(cell), F, T, _p(pheno), opt(use), K, opt(cov),
                                           P, opt(perm), _p(o["lod"]), _p(o["df"]), opt(o["slope"]), _p(o["rss0"]), _p(o["n_used"]),
                                           _p(o["n_cells"]), opt(o["perm_max"]), flags), "cnf2_qtl_scan_fam")
        return o

    def qtl_scan_fam(self, origin, side, grp, n_fam, pheno, cell=None, cov=None, use=None, perm=None, slopes=False, out=None):
        """cnf2_qtl_scan_fam on host rows origin[n][M][4]: the nested half-sib model -- a mean per cell[n] (None: grp) and a
        substitution effect per slope group grp[n] (0 .. n_fam-1 the F1 parent on the side, < 0 not nested) on bit 0 (side 0) or
        bit 3 (side 1) of the origin rows.  A dict: lod[T][M], df[M] (the fitted families), slope[T][M][F] with slopes (NaN for
        a family that is not fitted), rss0[T][C], n_used[C], n_cells[C], perm_max[P][T][C] (None without permutations).  The
        model: include/cnf2hip.h; cnf2freq_amd/qtl.py (families, scan_fam, fam_fstat) makes the groups and reads the results."""
        origin = self._origin_rows(origin)
        return self._qtlfam_call(origin.shape[0], _p(origin), side, grp, cell, n_fam, pheno, cov, use, perm, slopes, 0, out)

    def qtl_scan_fam_device(self, n, d_origin, side, grp, n_fam, pheno, cell=None, cov=None, use=None, perm=None, slopes=False,
                            d_out=None):
        """The same on device rows (d_origin as qtl_scan_device's).  d_out: a dict of device pointers (ints) for QTLFAM_KEYS
        (slope and perm_max None where not asked for) -- the outputs then stay on the GPU and None is returned."""
        if d_out is None:
            return self._qtlfam_call(n, C.c_void_p(d_origin), side, grp, cell, n_fam, pheno, cov, use, perm, slopes, QTL_ORIGIN_DEVICE)
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        grp = np.ascontiguousarray(grp, np.int32)
        cell = None if cell is None else np.ascontiguousarray(cell, np.int32)
        opt = lambda a: None if a is None else _p(a)
        dp = lambda k: C.c_void_p(d_out[k]) if d_out.get(k) else None
        self._chk(self.L.cnf2_qtl_scan_fam(self.h, n, C.c_void_p(d_origin), int(side), _p(grp), opt(cell), int(n_fam), T, _p(pheno),
                                           opt(use), K, opt(cov), P, opt(perm), dp("lod"), dp("df"), dp("slope"), dp("rss0"),
                                           dp("n_used"), dp("n_cells"), dp("perm_max"), QTL_ORIGIN_DEVICE | OUT_DEVICE),
                  "cnf2_qtl_scan_fam")
        return None

    # -- founder-haplotype scan ---------------------------------------------------
    QTLHAP_KEYS = ("lod", "df", "coef", "rss0", "n_used", "perm_max")

    def _qtlhap_call(self, n, descent_ptr, col, H, pheno, cov, use, perm, coef, flags, d_out=None):
        """cnf2_qtl_scan_hap on the rows behind descent_ptr, with new host outputs or (d_out) device pointers"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        col = np.ascontiguousarray(col, np.int32)
        if col.shape != (n, 8):
            raise ValueError("col must be [n][8]")
        M, Cn, H = self.n_markers, self.n_chrom, int(H)
        opt = lambda a: None if a is None else _p(a)
        if d_out is not None:
            dp = lambda k: C.c_void_p(d_out[k]) if d_out.get(k) else None
            self._chk(self.L.cnf2_qtl_scan_hap(self.h, n, descent_ptr, _p(col), H, T, _p(pheno), opt(use), K, opt(cov), P, opt(perm),
                                               dp("lod"), dp("df"), dp("coef"), dp("rss0"), dp("n_used"), dp("perm_max"),
                                               flags | OUT_DEVICE), "cnf2_qtl_scan_hap")
            return None
        o = dict(lod=np.zeros((T, M)), df=np.zeros(M, np.int32), coef=np.zeros((T, M, max(H, 0))) if coef else None,
                 rss0=np.zeros((T, Cn)), n_used=np.zeros(Cn, np.int32), perm_max=np.zeros((P, T, Cn)) if P else None)
        self._chk(self.L.cnf2_qtl_scan_hap(self.h, n, descent_ptr, _p(col), H, T, _p(pheno), opt(use), K, opt(cov), P, opt(perm),
                                           _p(o["lod"]), _p(o["df"]), opt(o["coef"]), _p(o["rss0"]), _p(o["n_used"]),
                                           opt(o["perm_max"]), flags), "cnf2_qtl_scan_hap")
        return o

    def qtl_scan_hap(self, descent, col, n_columns, pheno, cov=None, use=None, perm=None, coef=True):
        """cnf2_qtl_scan_hap on host rows descent[n][M][8] (what sweep_descent returns): the regression of pheno[n][T] on the
        expected dosage of the n_columns (1 .. 32) founder haplotypes that col[n][8] (origins.descent_columns) assigns the cells
        of a row to.  A dict: lod[T][M], df[M] (the columns kept), coef[T][M][H] with coef (NaN for a dropped column), rss0[T][C],
        n_used[C], perm_max[P][T][C] (None without permutations).  The model: include/cnf2hip.h; cnf2freq_amd/qtl.py (scan_hap,
        hap_fstat) makes the columns and reads the results."""
        descent = np.ascontiguousarray(descent, np.float64)
        if descent.ndim != 3 or descent.shape[1:] != (self.n_markers, 8):
            raise ValueError("descent must be [n][%d][8]" % self.n_markers)
        return self._qtlhap_call(descent.shape[0], _p(descent), col, n_columns, pheno, cov, use, perm, coef, 0)

    def qtl_scan_hap_device(self, n, d_descent, col, n_columns, pheno, cov=None, use=None, perm=None, coef=True, d_out=None):
        """The same on device rows (d_descent: an int, the pointer of n x M x 8 doubles aligned to 16 bytes, e.g. the tensor a
        sweep_descent_device call filled); they are read in place.  d_out: a dict of device pointers (ints) for QTLHAP_KEYS
        (coef and perm_max None where not asked for) -- the outputs then stay on the GPU and None is returned."""
        return self._qtlhap_call(n, C.c_void_p(d_descent), col, n_columns, pheno, cov, use, perm, coef, QTL_ORIGIN_DEVICE, d_out)

    # -- variance-component scan ---------------------------------------------------
    QTLVC_KEYS = ("lod", "h", "sigma2", "blup", "eval", "rank", "rss0", "n_used", "perm_max")

    def _qtlvc_call(self, n, descent_ptr, col, H, pheno, cov, use, perm, blup, evals, flags, d_out=None):
        """cnf2_qtl_scan_vc on the rows behind descent_ptr, with new host outputs or (d_out) device pointers"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        col = np.ascontiguousarray(col, np.int32)
        if col.shape != (n, 8):
            raise ValueError("col must be [n][8]")
        M, Cn, H = self.n_markers, self.n_chrom, int(H)
        opt = lambda a: None if a is None else _p(a)
        if d_out is not None:
            dp = lambda k: C.c_void_p(d_out[k]) if d_out.get(k) else None
            self._chk(self.L.cnf2_qtl_scan_vc(self.h, n, descent_ptr, _p(col), H, T, _p(pheno), opt(use), K, opt(cov), P, opt(perm),
                                              *[dp(k) for k in self.QTLVC_KEYS], flags | OUT_DEVICE), "cnf2_qtl_scan_vc")
            return None
        Hs = max(H, 0)
        o = dict(lod=np.zeros((T, M)), h=np.zeros((T, M)), sigma2=np.zeros((T, M)), blup=np.zeros((T, M, Hs)) if blup else None,
                 eval=np.zeros((M, Hs)) if evals else None, rank=np.zeros(M, np.int32), rss0=np.zeros((T, Cn)),
                 n_used=np.zeros(Cn, np.int32), perm_max=np.zeros((P, T, Cn)) if P else None)
        self._chk(self.L.cnf2_qtl_scan_vc(self.h, n, descent_ptr, _p(col), H, T, _p(pheno), opt(use), K, opt(cov), P, opt(perm),
                                          *[opt(o[k]) for k in self.QTLVC_KEYS], flags), "cnf2_qtl_scan_vc")
        return o

    def qtl_scan_vc(self, descent, col, n_columns, pheno, cov=None, use=None, perm=None, blup=True, evals=True):
        """cnf2_qtl_scan_vc on host rows descent[n][M][8] (what sweep_descent returns): the variance-component scan of pheno[n][T]
        with random effects of the n_columns (1 .. 64) founder haplotypes that col[n][8] (origins.descent_columns) assigns the
        cells of a row to.  A dict: lod[T][M], h[T][M] (s_u^2 / (s_u^2 + s_e^2)), sigma2[T][M] (s_e^2), blup[T][M][H] with blup,
        eval[M][H] with evals (the eigenvalues of the marker's W, descending), rank[M], rss0[T][C], n_used[C], perm_max[P][T][C]
        (None without permutations).  The model: include/cnf2hip.h; cnf2freq_amd/qtl.py (scan_vc) makes the columns."""
        descent = np.ascontiguousarray(descent, np.float64)
        if descent.ndim != 3 or descent.shape[1:] != (self.n_markers, 8):
            raise ValueError("descent must be [n][%d][8]" % self.n_markers)
        return self._qtlvc_call(descent.shape[0], _p(descent), col, n_columns, pheno, cov, use, perm, blup, evals, 0)

    def qtl_scan_vc_device(self, n, d_descent, col, n_columns, pheno, cov=None, use=None, perm=None, blup=True, evals=True, d_out=None):
        """The same on device rows (d_descent: an int, the pointer of n x M x 8 doubles aligned to 16 bytes); they are read in
        place.  d_out: a dict of device pointers (ints) for QTLVC_KEYS (blup, eval and perm_max None where not asked for) -- the
        outputs then stay on the GPU and None is returned."""
        return self._qtlvc_call(n, C.c_void_p(d_descent), col, n_columns, pheno, cov, use, perm, blup, evals, QTL_ORIGIN_DEVICE, d_out)

    # -- multiple-imputation scan ------------------------------------------------
    def set_qtlimp_columns(self, cap):
        """Cap on the phenotype columns per tile of qtl_scan_imp (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtlimp_columns(self.h, cap), "cnf2_set_qtlimp_columns")

    def sweep_sample_device(self, ind_begin, ind_end, draws, seed, d_factors, d_loglik, d_state, d_shift, d_logp=None, flags=0):
        """cnf2_sweep_sample in its device-pointer form (ints; d_logp may be None): the states stay on the GPU, where
        qtl_scan_imp_device reads them in place."""
        self._chk(self.L.cnf2_sweep_sample(self.h, ind_begin, ind_end, draws, int(seed) & 0xFFFFFFFFFFFFFFFF, C.c_void_p(d_factors),
                                           C.c_void_p(d_loglik), C.c_void_p(d_state), C.c_void_p(d_shift),
                                           C.c_void_p(d_logp) if d_logp else None, flags | OUT_DEVICE), "cnf2_sweep_sample")

    QTLIMP_KEYS = ("lod", "coef", "rank", "rss0", "n_used", "perm_max", "draw_lod")

    def _qtlimp_call(self, n, D, state_ptr, pheno, cov, use, perm, draw_lods, flags, out=None):
        """cnf2_qtl_scan_imp on the states behind state_ptr; out = None: new host arrays, else the outputs (arrays, or with
        OUT_DEVICE in flags ints, the device pointers; perm_max / draw_lod None where not asked for)"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        if out is None:
            out = self._qtl_outputs(T, P)
            out["draw_lod"] = np.zeros((D, T, self.n_markers)) if draw_lods else None
        opt = lambda a: None if a is None else _p(a)
        ptr = (lambda a: C.c_void_p(a) if a else None) if flags & OUT_DEVICE else opt
        self._chk(self.L.cnf2_qtl_scan_imp(self.h, n, D, state_ptr, T, _p(pheno), opt(use), K, opt(cov), P, opt(perm),
                                           *[ptr(out.get(k)) for k in self.QTLIMP_KEYS], flags), "cnf2_qtl_scan_imp")
        return out

    def qtl_scan_imp(self, state, pheno, cov=None, use=None, perm=None, additive=False, draw_lods=False, out=None):
        """cnf2_qtl_scan_imp on host states state[n][D][M] (uint8, what sweep_sample returns): the model of qtl_scan fitted to
        the hard origin classes of every draw and the draws combined per (marker, column) on the likelihood scale --
        lod = log10 of the mean of 10^lod_d, coef the mean of the draws' effects weighted with 10^lod_d (NaN once a draw drops
        the column), rank the smallest over the draws.  The dict of qtl_scan (perm_max[P][T][C] the largest combined LOD) plus
        draw_lod[D][T][M], the draws' own profiles, with draw_lods (else None).  The model: include/cnf2hip.h."""
        state = np.ascontiguousarray(state, np.uint8)
        if state.ndim != 3 or state.shape[2] != self.n_markers:
            raise ValueError("state must be [n][D][%d]" % self.n_markers)
        return self._qtlimp_call(state.shape[0], state.shape[1], _p(state), pheno, cov, use, perm, draw_lods,
                                 QTL_ADDITIVE if additive else 0, out)

    def qtl_scan_imp_device(self, n, draws, d_state, pheno, cov=None, use=None, perm=None, additive=False, draw_lods=False,
                            d_out=None):
        """The same on device states (d_state: an int, the pointer of n x draws x M bytes, e.g. the tensor a
        sweep_sample_device call filled); they are read in place.  Phenotypes are host arrays.  With d_out (a dict of device
        pointers under QTLIMP_KEYS; perm_max None without permutations, draw_lod None or absent when not wanted) the outputs
        are written there and the call returns d_out; else host arrays as qtl_scan_imp."""
        flags = QTL_STATE_DEVICE | (QTL_ADDITIVE if additive else 0) | (OUT_DEVICE if d_out is not None else 0)
        return self._qtlimp_call(n, draws, C.c_void_p(d_state), pheno, cov, use, perm, draw_lods, flags, d_out)

    # -- kinship sums and the column scan (the two halves of a mixed-model scan: cnf2freq_amd/qtl.py) ----
    def kinship_sums(self, origin, chrom_begin=0, chrom_end=None):
        """cnf2_kinship_sums on host rows origin[n][M][4]: (sum[n][n], markers) with sum[i][j] the sum of a_i(m) a_j(m),
        a = origin[3] - origin[0], over the markers of the chromosomes chrom_begin .. chrom_end-1 (None: to the last).  The
        kinship is K = (1 + sum / markers) / 2; leaving a chromosome out is a subtraction of sums (qtl.kinship)."""
        origin = self._origin_rows(origin)
        n = origin.shape[0]
        out, cnt = np.zeros((n, n)), np.zeros(1, np.int32)
        chrom_end = self.n_chrom if chrom_end is None else chrom_end
        self._chk(self.L.cnf2_kinship_sums(self.h, n, _p(origin), chrom_begin, chrom_end, _p(out), _p(cnt), 0), "cnf2_kinship_sums")
        return out, int(cnt[0])

    def kinship_sums_device(self, n, d_origin, chrom_begin=0, chrom_end=None, d_sum=None, d_n_markers=None):
        """The same on device rows (d_origin: an int, the pointer of n x M x 4 doubles aligned to 16 bytes; None: the rows this
        context's last sweep_qtl left in it), read in place.  With d_sum and d_n_markers (ints: n x n doubles, one int32) the
        outputs are device memory and the call returns None; else (sum[n][n], markers) as host values."""
        chrom_end = self.n_chrom if chrom_end is None else chrom_end
        origin = C.c_void_p(d_origin) if d_origin else None
        if d_sum:
            self._chk(self.L.cnf2_kinship_sums(self.h, n, origin, chrom_begin, chrom_end, C.c_void_p(d_sum), C.c_void_p(d_n_markers),
                                               QTL_ORIGIN_DEVICE | OUT_DEVICE), "cnf2_kinship_sums")
            return None
        out, cnt = np.zeros((n, n)), np.zeros(1, np.int32)
        self._chk(self.L.cnf2_kinship_sums(self.h, n, origin, chrom_begin, chrom_end, _p(out), _p(cnt), QTL_ORIGIN_DEVICE),
                  "cnf2_kinship_sums")
        return out, int(cnt[0])

    def _qtl_cols_call(self, n, M, ne, reg_ptr, x0, pheno, scale, perm, flags, out=None):
        """cnf2_qtl_scan_cols with host outputs (out = None: new arrays) on the regressors behind reg_ptr"""
        pheno, _, _, perm = self._qtl_inputs(n, pheno, None, None, perm)
        x0 = np.ascontiguousarray(x0, np.float64)
        x0 = x0[:, None] if x0.ndim == 1 else x0
        if x0.ndim != 2 or x0.shape[0] != n:
            raise ValueError("x0 must be [n][nx]")
        if scale is not None:
            scale = np.ascontiguousarray(scale, np.float64)
            if scale.shape != (n,):
                raise ValueError("scale must be [n]")
        T, P = pheno.shape[1], 0 if perm is None else perm.shape[0]
        o = dict(lod=np.zeros((T, M)), coef=np.zeros((T, M, 2)), rank=np.zeros(M, np.int32), rss0=np.zeros(T),
                 perm_max=np.zeros((P, T)) if P else None) if out is None else out
        opt = lambda a: None if a is None else _p(a)
        self._chk(self.L.cnf2_qtl_scan_cols(self.h, n, M, ne, reg_ptr, opt(scale), x0.shape[1], _p(x0), T, _p(pheno), P, opt(perm),
                                            _p(o["lod"]), _p(o["coef"]), _p(o["rank"]), _p(o["rss0"]), opt(o["perm_max"]), flags),
                  "cnf2_qtl_scan_cols")
        return o

    def qtl_scan_cols(self, reg, x0, pheno, scale=None, perm=None, out=None):
        """cnf2_qtl_scan_cols on host regressors reg[n][M][ne] (ne = 1 or 2): least squares of every column of pheno[n][T],
        observed and permuted by perm[P][n], on [x0, scale_i reg(i, m)] at every marker of the block.  x0[n][nx] is the whole
        null design -- no intercept is added and nothing is centred -- and scale[n] (None: ones) multiplies the regressor rows
        on the fly.  A dict: lod[T][M], coef[T][M][2] (NaN for a dropped column), rank[M], rss0[T], perm_max[P][T] (None
        without permutations).  The model: include/cnf2hip.h; qtl.scan_lmm uses it on rotated columns."""
        reg = np.ascontiguousarray(reg, np.float64)
        reg = reg[:, :, None] if reg.ndim == 2 else reg
        if reg.ndim != 3 or reg.shape[2] not in (1, 2):
            raise ValueError("reg must be [n][M][ne] with ne = 1 or 2")
        return self._qtl_cols_call(reg.shape[0], reg.shape[1], reg.shape[2], _p(reg), x0, pheno, scale, perm, 0, out)

    def qtl_scan_cols_device(self, n, n_mark, ne, d_reg, x0, pheno, scale=None, perm=None):
        """The same on device regressors (d_reg: an int, the pointer of n x n_mark x ne doubles aligned to 16 bytes), read in
        place.  x0, pheno, scale, perm and the outputs are host arrays."""
        return self._qtl_cols_call(n, n_mark, ne, C.c_void_p(d_reg), x0, pheno, scale, perm, QTL_REG_DEVICE)

    # -- bootstrap scan --------------------------------------------------------------
    def _qtl_boot_call(self, n, origin_ptr, pheno, count, chrom_begin, chrom_end, cov, use, profile, flags, out=None):
        """cnf2_qtl_scan_boot with host outputs (out = None: new arrays) on the rows behind origin_ptr"""
        pheno, cov, use, _ = self._qtl_inputs(n, pheno, cov, use, None)
        count = np.ascontiguousarray(count, np.int32)
        count = count[None, :] if count.ndim == 1 else count
        if count.ndim != 2 or count.shape[1] != n:
            raise ValueError("count must be [B][n]")
        chrom_end = self.n_chrom if chrom_end is None else chrom_end
        if not 0 <= chrom_begin < chrom_end <= self.n_chrom:
            raise ValueError("the chromosome range must be non-empty and within 0 .. %d" % self.n_chrom)
        T, K, B = pheno.shape[1], 0 if cov is None else cov.shape[1], count.shape[0]
        Cn = chrom_end - chrom_begin
        Mn = int(self.chromstarts[chrom_end] - self.chromstarts[chrom_begin])
        o = dict(boot_max=np.zeros((B, T, Cn)), boot_arg=np.zeros((B, T, Cn), np.int32), n_boot=np.zeros((B, Cn), np.int32),
                 boot_lod=np.zeros((B, T, Mn)) if profile else None) if out is None else out
        opt = lambda a: None if a is None else _p(a)
        self._chk(self.L.cnf2_qtl_scan_boot(self.h, n, origin_ptr, T, _p(pheno), opt(use), K, opt(cov), chrom_begin, chrom_end, B,
                                            _p(count), _p(o["boot_max"]), _p(o["boot_arg"]), _p(o["n_boot"]), opt(o["boot_lod"]),
                                            flags), "cnf2_qtl_scan_boot")
        return o

    def qtl_scan_boot(self, origin, pheno, count, chrom_begin=0, chrom_end=None, cov=None, use=None, additive=False,
                      profile=False, out=None):
        """cnf2_qtl_scan_boot on host rows origin[n][M][4]: the scan of qtl_scan on resampled individuals.  count[B][n] (int32)
        says how often replicate b draws individual i (qtl.bootstrap_counts); the chromosomes chrom_begin .. chrom_end-1
        (None: to the last) are scanned.  A dict: boot_max[B][T][C'] the largest LOD of each chromosome, boot_arg[B][T][C']
        the marker that has it (the lowest among equal ones; -1 and a maximum of 0 where the replicate cannot be fitted),
        n_boot[B][C'] the individuals drawn, counted as often as drawn, and with profile boot_lod[B][T][M'] (else None).
        The model: include/cnf2hip.h; qtl.boot_interval reads boot_arg."""
        origin = self._origin_rows(origin)
        return self._qtl_boot_call(origin.shape[0], _p(origin), pheno, count, chrom_begin, chrom_end, cov, use, profile,
                                   QTL_ADDITIVE if additive else 0, out)

    def qtl_scan_boot_device(self, n, d_origin, pheno, count, chrom_begin=0, chrom_end=None, cov=None, use=None, additive=False,
                             profile=False, out=None):
        """The same on device rows (d_origin: an int, the pointer of n x M x 4 doubles aligned to 16 bytes), read in place;
        d_origin None: the rows this context's last sweep_qtl left in it, which stay valid.  Phenotypes, counts and outputs
        are host arrays."""
        return self._qtl_boot_call(n, C.c_void_p(d_origin) if d_origin else None, pheno, count, chrom_begin, chrom_end, cov, use,
                                   profile, QTL_ORIGIN_DEVICE | (QTL_ADDITIVE if additive else 0), out)

    # -- multi-trait scan --------------------------------------------------------------
    QTLMV_KEYS = ("lod", "rank", "trait_rank", "n_used", "perm_max")

    def set_qtlmv_groups(self, cap):
        """Cap on the groups (the observed data, every permutation) per tile of qtl_scan_mv (0 = what memory allows); results
        do not depend on it."""
        self._chk(self.L.cnf2_set_qtlmv_groups(self.h, cap), "cnf2_set_qtlmv_groups")

    def _qtlmv_call(self, n, origin_ptr, pheno, cov, use, perm, flags, out=None):
        """cnf2_qtl_scan_mv on the rows behind origin_ptr; out = None: new host arrays, else the outputs (arrays, or with
        OUT_DEVICE in flags ints, the device pointers)"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        M, Cn = self.n_markers, self.n_chrom
        o = dict(lod=np.zeros(M), rank=np.zeros(M, np.int32), trait_rank=np.zeros(Cn, np.int32), n_used=np.zeros(Cn, np.int32),
                 perm_max=np.zeros((P, Cn)) if P else None) if out is None else out
        opt = lambda a: None if a is None else _p(a)
        ptr = (lambda a: C.c_void_p(a) if a else None) if flags & OUT_DEVICE else opt
        self._chk(self.L.cnf2_qtl_scan_mv(self.h, n, origin_ptr, T, _p(pheno), opt(use), K, opt(cov), P, opt(perm),
                                          *[ptr(o[k]) for k in self.QTLMV_KEYS], flags), "cnf2_qtl_scan_mv")
        return o

    def qtl_scan_mv(self, origin, pheno, cov=None, use=None, perm=None, additive=False, out=None):
        """cnf2_qtl_scan_mv on host rows origin[n][M][4]: the joint LOD (Wilks' lambda) of the T <= 16 traits pheno[n][T] on
        the rows at every marker, with covariates cov[n][K], the individuals of use[n] and the permutations perm[P][n], each of
        which moves all traits of an individual together.  A dict: lod[M], rank[M], trait_rank[C] (the traits kept),
        n_used[C], perm_max[P][C] (None without permutations).  The model: include/cnf2hip.h; qtl.scan_mv reads it."""
        origin = self._origin_rows(origin)
        return self._qtlmv_call(origin.shape[0], _p(origin), pheno, cov, use, perm, QTL_ADDITIVE if additive else 0, out)

    def qtl_scan_mv_device(self, n, d_origin, pheno, cov=None, use=None, perm=None, additive=False, d_out=None):
        """The same on device rows (d_origin: an int, the pointer of n x M x 4 doubles aligned to 16 bytes), read in place;
        d_origin None: the rows this context's last sweep_qtl left in it, which stay valid.  Phenotypes are host arrays.
        d_out: a dict of device pointers (ints) under the keys of QTLMV_KEYS, perm_max None without permutations -- the
        outputs are written there and the call returns d_out; else host arrays as qtl_scan_mv."""
        flags = QTL_ORIGIN_DEVICE | (QTL_ADDITIVE if additive else 0) | (OUT_DEVICE if d_out is not None else 0)
        return self._qtlmv_call(n, C.c_void_p(d_origin) if d_origin else None, pheno, cov, use, perm, flags, d_out)

    # -- two-QTL pair scan ---------------------------------------------------------
    QTL2_KEYS = ("lod_add", "lod_full", "rank_add", "rank_full", "rss0", "n_used", "perm_max")

    def set_qtl2_columns(self, cap):
        """Cap on the phenotype columns per tile of qtl_scan2 (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtl2_columns(self.h, cap), "cnf2_set_qtl2_columns")

    def _qtl2_outputs(self, T, P, L):
        Cn = self.n_chrom
        return dict(lod_add=np.zeros((T, L, L)), lod_full=np.zeros((T, L, L)), rank_add=np.zeros((L, L), np.int32),
                    rank_full=np.zeros((L, L), np.int32), rss0=np.zeros((T, Cn, Cn)), n_used=np.zeros((Cn, Cn), np.int32),
                    perm_max=np.zeros((P, T, 3)) if P else None)

    def _qtl2_call(self, n, origin_ptr, sel, pheno, cov, use, perm, flags, out=None, joint_ptr=None):
        """cnf2_qtl_scan2 -- with joint_ptr cnf2_qtl_scan2_linked -- with host outputs (out = None: new arrays) on the rows
        behind origin_ptr"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        sel = np.ascontiguousarray(sel, np.int32)
        if sel.ndim != 1:
            raise ValueError("sel must be [L]")
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        o = self._qtl2_outputs(T, P, len(sel)) if out is None else out
        opt = lambda a: None if a is None else _p(a)
        outs = (_p(o["lod_add"]), _p(o["lod_full"]), _p(o["rank_add"]), _p(o["rank_full"]), _p(o["rss0"]), _p(o["n_used"]),
                opt(o["perm_max"]), flags)
        if joint_ptr is None:
            self._chk(self.L.cnf2_qtl_scan2(self.h, n, origin_ptr, len(sel), _p(sel), T, _p(pheno), opt(use), K, opt(cov), P,
                                            opt(perm), *outs), "cnf2_qtl_scan2")
        else:
            self._chk(self.L.cnf2_qtl_scan2_linked(self.h, n, origin_ptr, joint_ptr, len(sel), _p(sel), T, _p(pheno), opt(use), K,
                                                   opt(cov), P, opt(perm), *outs), "cnf2_qtl_scan2_linked")
        return o

    def qtl_scan2_linked(self, origin, joint, sel, pheno, cov=None, use=None, perm=None, additive=False):
        """cnf2_qtl_scan2_linked on host rows origin[n][M][4] and joint[n][n_pairs][16] (sweep_pairs' rows for the same sel):
        qtl_scan2, with the full model fitted on the pairs of one chromosome too -- there the interaction columns are the
        expectations of the products under the joint -- and perm_max[..][1], [..][2] over all pairs."""
        origin = self._origin_rows(origin)
        joint = np.ascontiguousarray(joint, np.float64)
        if joint.ndim != 3 or joint.shape[0] != origin.shape[0] or joint.shape[2] != 16:
            raise ValueError("joint must be [n][n_pairs][16] with n = %d" % origin.shape[0])
        return self._qtl2_call(origin.shape[0], _p(origin), sel, pheno, cov, use, perm, QTL_ADDITIVE if additive else 0,
                               joint_ptr=_p(joint))

    def qtl_scan2_linked_device(self, n, d_origin, d_joint, sel, pheno, cov=None, use=None, perm=None, additive=False):
        """The same on device rows and a device joint, both read in place."""
        return self._qtl2_call(n, C.c_void_p(d_origin), sel, pheno, cov, use, perm,
                               QTL_ORIGIN_DEVICE | QTL_JOINT_DEVICE | (QTL_ADDITIVE if additive else 0), joint_ptr=C.c_void_p(d_joint))

    def qtl_scan2(self, origin, sel, pheno, cov=None, use=None, perm=None, additive=False):
        """cnf2_qtl_scan2 on host rows origin[n][M][4]: for every pair j < k of the markers sel[L] (strictly ascending) the
        additive-pair and the full (epistatic) Haley-Knott model of pheno[n][T], with covariates cov[n][K], K <= 6, the
        individuals of use[n] and the permutations perm[P][n].  A dict: lod_add[T][L][L], lod_full[T][L][L] (NaN for a pair
        on one chromosome), rank_add[L][L], rank_full[L][L] -- cells j < k only, the others NaN / -1 -- rss0[T][C][C],
        n_used[C][C], perm_max[P][T][3] (the maxima of lod_add, lod_full and lod_full - lod_add; None without
        permutations).  The model: include/cnf2hip.h; cnf2freq_amd/qtl.py reads the results."""
        origin = self._origin_rows(origin)
        return self._qtl2_call(origin.shape[0], _p(origin), sel, pheno, cov, use, perm, QTL_ADDITIVE if additive else 0)

    def qtl_scan2_device(self, n, d_origin, sel, pheno, cov=None, use=None, perm=None, additive=False):
        """The same on device rows, read in place (d_origin as for qtl_scan_device; None: the rows this context's last
        sweep_qtl left in it, which this call leaves valid)."""
        return self._qtl2_call(n, C.c_void_p(d_origin), sel, pheno, cov, use, perm,
                               QTL_ORIGIN_DEVICE | (QTL_ADDITIVE if additive else 0))

    # -- extended single-locus scan: imprinting and QTL x covariate interaction ------
    QTLX_KEYS = ("lod", "coef", "rank", "rss0", "n_used", "perm_max")

    def set_qtlx_columns(self, cap):
        """Cap on the phenotype columns per tile of qtl_scanx (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtlx_columns(self.h, cap), "cnf2_set_qtlx_columns")

    def _qtlx_outputs(self, T, P, ncoef):
        M, Cn = self.n_markers, self.n_chrom
        return dict(lod=np.zeros((T, M, 3)), coef=np.zeros((T, M, ncoef)), rank=np.zeros((M, 3), np.int32), rss0=np.zeros((T, Cn)),
                    n_used=np.zeros(Cn, np.int32), perm_max=np.zeros((P, T, Cn, 5)) if P else None)

    def _qtlx_call(self, n, origin_ptr, pheno, cov, interactive, use, perm, flags, out=None):
        """cnf2_qtl_scanx with host outputs (out = None: new arrays) on the rows behind origin_ptr"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        o = self._qtlx_outputs(T, P, self._n_effects(flags) * (1 + max(0, int(interactive)))) if out is None else out
        opt = lambda a: None if a is None else _p(a)
        self._chk(self.L.cnf2_qtl_scanx(self.h, n, origin_ptr, T, _p(pheno), opt(use), K, opt(cov), int(interactive), P, opt(perm),
                                        _p(o["lod"]), _p(o["coef"]), _p(o["rank"]), _p(o["rss0"]), _p(o["n_used"]),
                                        opt(o["perm_max"]), flags), "cnf2_qtl_scanx")
        return o

    def qtl_scanx(self, origin, pheno, cov=None, interactive=0, imprint=False, use=None, perm=None, additive=False, out=None):
        """cnf2_qtl_scanx on host rows origin[n][M][4]: per marker the nested Haley-Knott models Mendelian (a, d), imprinting
        (+ i = o[1] - o[2], with imprint) and interaction (+ the products of every effect with the first `interactive`
        columns of cov[n][K]) of pheno[n][T], with the individuals of use[n] and the permutations perm[P][n].  A dict:
        lod[T][M][3] (nested, non-decreasing), coef[T][M][ne (1 + interactive)] (the full model's effects, NaN for a dropped
        column), rank[M][3] (cumulative), rss0[T][C], n_used[C], perm_max[P][T][C][5] (the maxima of the three LODs, of
        lod[1] - lod[0] and of lod[2] - lod[1]; None without permutations).  The model: include/cnf2hip.h;
        cnf2freq_amd/qtl.py reads the results."""
        origin = self._origin_rows(origin)
        return self._qtlx_call(origin.shape[0], _p(origin), pheno, cov, interactive, use, perm,
                               (QTL_ADDITIVE if additive else 0) | (QTL_IMPRINT if imprint else 0), out)

    def qtl_scanx_device(self, n, d_origin, pheno, cov=None, interactive=0, imprint=False, use=None, perm=None, additive=False):
        """The same on device rows, read in place (d_origin as for qtl_scan_device; None: the rows this context's last
        sweep_qtl left in it, which this call leaves valid)."""
        return self._qtlx_call(n, C.c_void_p(d_origin), pheno, cov, interactive, use, perm,
                               QTL_ORIGIN_DEVICE | (QTL_ADDITIVE if additive else 0) | (QTL_IMPRINT if imprint else 0))

    # -- cofactor scan: composite interval mapping, multi-QTL fits --------------------
    QTLCOF_KEYS = ("lod", "lod_base", "coef", "rank", "rank_cof", "rss0", "n_used", "perm_max")

    def set_qtlcof_columns(self, cap):
        """Cap on the phenotype columns per tile of qtl_scan_cof (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtlcof_columns(self.h, cap), "cnf2_set_qtlcof_columns")

    def _qtlcof_outputs(self, T, P, ne):
        M, Cn = self.n_markers, self.n_chrom
        return dict(lod=np.zeros((T, M)), lod_base=np.zeros((T, M)), coef=np.zeros((T, M, ne)), rank=np.zeros(M, np.int32),
                    rank_cof=np.zeros(M, np.int32), rss0=np.zeros((T, Cn)), n_used=np.zeros(Cn, np.int32),
                    perm_max=np.zeros((P, T, Cn)) if P else None)

    @staticmethod
    def _qtlcof_ranges(cof, excl):
        """(cof, excl_lo, excl_hi) as int32 arrays [Q]; excl None: every cofactor is left out at its own marker only"""
        cof = np.ascontiguousarray([] if cof is None else cof, np.int32).reshape(-1)
        lo, hi = (cof, cof) if excl is None else excl
        lo, hi = np.ascontiguousarray(lo, np.int32).reshape(-1), np.ascontiguousarray(hi, np.int32).reshape(-1)
        if lo.shape != cof.shape or hi.shape != cof.shape:
            raise ValueError("excl must be (excl_lo[Q], excl_hi[Q]) with Q = len(cof)")
        return cof, lo.copy(), hi.copy()

    def _qtlcof_call(self, n, origin_ptr, pheno, cof, excl, cov, use, perm, flags, out=None):
        """cnf2_qtl_scan_cof with host outputs (out = None: new arrays) on the rows behind origin_ptr"""
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        cof, lo, hi = self._qtlcof_ranges(cof, excl)
        T, K, P = pheno.shape[1], 0 if cov is None else cov.shape[1], 0 if perm is None else perm.shape[0]
        o = self._qtlcof_outputs(T, P, 1 if flags & QTL_ADDITIVE else 2) if out is None else out
        opt = lambda a: None if a is None else _p(a)
        self._chk(self.L.cnf2_qtl_scan_cof(self.h, n, origin_ptr, T, _p(pheno), opt(use), K, opt(cov), len(cof), _p(cof), _p(lo),
                                           _p(hi), P, opt(perm), _p(o["lod"]), _p(o["lod_base"]), _p(o["coef"]), _p(o["rank"]),
                                           _p(o["rank_cof"]), _p(o["rss0"]), _p(o["n_used"]), opt(o["perm_max"]), flags),
                  "cnf2_qtl_scan_cof")
        return o

    def qtl_scan_cof(self, origin, pheno, cof, excl=None, cov=None, use=None, perm=None, additive=False, out=None):
        """cnf2_qtl_scan_cof on host rows origin[n][M][4]: composite interval mapping.  Every marker is fitted together with
        the cofactors cof[Q] (marker indices, strictly ascending); cofactor q is left out of the design at the markers
        excl[0][q] .. excl[1][q] (excl None: at its own marker only; qtl.cofactor_windows makes ranges from a window in map
        units).  A dict: lod[T][M] (the conditional LOD of the marker given the cofactors), lod_base[T][M] (the cofactors
        against the null model), coef[T][M][ne] (the marker's effects in the full model, NaN for a dropped one), rank[M],
        rank_cof[M], rss0[T][C], n_used[C], perm_max[P][T][C] (the maxima over the markers in no range; None without
        permutations).  The model: include/cnf2hip.h; cnf2freq_amd/qtl.py reads the results."""
        origin = self._origin_rows(origin)
        return self._qtlcof_call(origin.shape[0], _p(origin), pheno, cof, excl, cov, use, perm, QTL_ADDITIVE if additive else 0, out)

    def qtl_scan_cof_device(self, n, d_origin, pheno, cof, excl=None, cov=None, use=None, perm=None, additive=False):
        """The same on device rows, read in place (d_origin as for qtl_scan_device; None: the rows this context's last
        sweep_qtl left in it, which this call leaves valid)."""
        return self._qtlcof_call(n, C.c_void_p(d_origin), pheno, cof, excl, cov, use, perm,
                                 QTL_ORIGIN_DEVICE | (QTL_ADDITIVE if additive else 0))

    def qtl_kept_rows(self, n, sel):
        """cnf2_qtl_kept_rows: [len(sel)][n][4], the rows this context's last sweep_qtl left in it at the markers sel"""
        sel = np.ascontiguousarray(sel, np.int32).reshape(-1)
        out = np.zeros((len(sel), n, 4))
        self._chk(self.L.cnf2_qtl_kept_rows(self.h, n, len(sel), _p(sel), _p(out)), "cnf2_qtl_kept_rows")
        return out

    # -- maximum-likelihood single-locus scan: EM interval mapping -------------------
    QTLEM_KEYS = ("lod", "coef", "sigma2", "iters", "status", "rank", "rss0", "n_used", "perm_max")

    def set_qtlem_columns(self, cap):
        """Cap on the phenotype columns per tile of qtl_scan_em (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtlem_columns(self.h, cap), "cnf2_set_qtlem_columns")

    # The four scans that fit a model by iteration per (marker, column) -- EM, binary, survival, variance -- are called on one
    # path, _qtlfit_call.  Per scan: the C function; the argument it takes beyond the shared ones ("status" behind the
    # times, "n_var" behind the covariates); its outputs in the order of the C arguments, which is the order of the dict,
    # each with its shape in letters -- T traits, M markers, C chromosomes, P permutations, E effects, 3 fits -- and dtype
    _F, _I = np.float64, np.int32
    _QTLFIT = dict(
        em=("cnf2_qtl_scan_em", None,
            (("lod", "TM", _F), ("coef", "TME", _F), ("sigma2", "TM", _F), ("iters", "TM", _I), ("status", "TM", _I),
             ("rank", "M", _I), ("rss0", "TC", _F), ("n_used", "C", _I), ("perm_max", "PTC", _F))),
        binary=("cnf2_qtl_scan_binary", None,
                (("lod", "TM", _F), ("coef", "TME", _F), ("iters", "TM", _I), ("status", "TM", _I), ("rank", "M", _I),
                 ("ll0", "TC", _F), ("n_ones", "TC", _I), ("n_used", "C", _I), ("perm_max", "PTC", _F))),
        surv=("cnf2_qtl_scan_surv", "status",
              (("lod", "TM", _F), ("coef", "TME", _F), ("iters", "TM", _I), ("status", "TM", _I), ("rank", "M", _I),
               ("ll0", "TC", _F), ("n_events", "TC", _I), ("n_used", "C", _I), ("perm_max", "PTC", _F))),
        var=("cnf2_qtl_scan_var", "n_var",
             (("lod", "TM3", _F), ("coef_mean", "TME", _F), ("coef_var", "TME", _F), ("iters", "TM3", _I), ("status", "TM3", _I),
              ("rank", "M", _I), ("ll0", "TC", _F), ("n_used", "C", _I), ("perm_max", "PTC3", _F))))

    def _qtlfit_call(self, scan, n, origin_ptr, pheno, cov, use, perm, max_iter, tol, flags, out=None, extra=None):
        """The C function of _QTLFIT[scan] on the rows behind origin_ptr, with host outputs (out = None: new arrays; else a
        dict of arrays), or with OUT_DEVICE in flags and out a dict of device pointers (ints; perm_max None without
        permutations).  extra: the scan's own argument (survival: status, with pheno the times; variance: n_var)."""
        name, own, outputs = self._QTLFIT[scan]
        pheno, cov, use, perm = self._qtl_inputs(n, pheno, cov, use, perm)
        opt = lambda a: None if a is None else _p(a)
        args = [self.h, n, origin_ptr, pheno.shape[1], _p(pheno)]
        if own == "status":
            extra = np.ascontiguousarray(extra, np.float64)
            extra = extra[:, None] if extra.ndim == 1 else extra
            if extra.shape != pheno.shape:
                raise ValueError("status must have the shape of time")
            args.append(_p(extra))
        args += [opt(use), 0 if cov is None else cov.shape[1], opt(cov)]
        if own == "n_var":
            args.append(int(extra))
        P = 0 if perm is None else perm.shape[0]
        dim = dict(T=pheno.shape[1], M=self.n_markers, C=self.n_chrom, P=P, E=self._n_effects(flags))
        if out is None:
            out = {key: np.zeros([dim[c] if c in dim else int(c) for c in shape], dtype) if P or key != "perm_max" else None
                   for key, shape, dtype in outputs}
        ptr = (lambda a: C.c_void_p(a) if a else None) if flags & OUT_DEVICE else opt
        self._chk(getattr(self.L, name)(*args, P, opt(perm), int(max_iter), float(tol), *[ptr(out[key]) for key, _, _ in outputs],
                                        flags), name)
        return out

    def qtl_scan_em(self, origin, pheno, cov=None, imprint=False, use=None, perm=None, additive=False, max_iter=1000, tol=1e-6,
                    out=None, flags=0):
        """cnf2_qtl_scan_em on host rows origin[n][M][4]: per marker the maximum-likelihood fit (EM interval mapping) of the
        normal mixture over the four origin classes to pheno[n][T], with the effects a, d (not with additive) and i (with
        imprint), covariates cov[n][K], the individuals of use[n] and the permutations perm[P][n].  A dict: lod[T][M],
        coef[T][M][ne] (NaN for a dropped effect), sigma2[T][M], iters[T][M], status[T][M] (0 = stopped by tol, 1 = by
        max_iter, 2 = breakdown), rank[M], rss0[T][C], n_used[C], perm_max[P][T][C] (None without permutations).  The model:
        include/cnf2hip.h; cnf2freq_amd/qtl.py reads the results."""
        origin = self._origin_rows(origin)
        return self._qtlfit_call("em", origin.shape[0], _p(origin), pheno, cov, use, perm, max_iter, tol,
                                 self._fit_flags(flags, additive, imprint), out)

    def qtl_scan_em_device(self, n, d_origin, pheno, cov=None, imprint=False, use=None, perm=None, additive=False, max_iter=1000,
                           tol=1e-6, out=None, flags=0):
        """The same on device rows, read in place (d_origin as for qtl_scan_device; None: the rows this context's last
        sweep_qtl left in it, which this call leaves valid).  With OUT_DEVICE in flags, out is a dict of device pointers."""
        return self._qtlfit_call("em", n, C.c_void_p(d_origin), pheno, cov, use, perm, max_iter, tol,
                                 self._fit_flags(flags | QTL_ORIGIN_DEVICE, additive, imprint), out)

    # -- binary-trait single-locus scan: logistic regression --------------------------
    def set_qtlbin_columns(self, cap):
        """Cap on the phenotype columns per tile of qtl_scan_binary (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtlbin_columns(self.h, cap), "cnf2_set_qtlbin_columns")

    def qtl_scan_binary(self, origin, pheno, cov=None, imprint=False, use=None, perm=None, additive=False, max_iter=50, tol=1e-7,
                        out=None, flags=0):
        """cnf2_qtl_scan_binary on host rows origin[n][M][4]: per marker the logistic regression of the 0/1 columns pheno[n][T]
        on the covariates cov[n][K] and the effects a, d (not with additive) and i (with imprint), by Newton's method from the
        null fit, for the individuals of use[n] and the permutations perm[P][n].  A dict: lod[T][M], coef[T][M][ne] (NaN for a
        dropped effect), iters[T][M], status[T][M] (0 = stopped by tol, 1 = by max_iter, 2 = breakdown), rank[M], ll0[T][C],
        n_ones[T][C], n_used[C], perm_max[P][T][C] (None without permutations).  The model: include/cnf2hip.h;
        cnf2freq_amd/qtl.py reads the results."""
        origin = self._origin_rows(origin)
        return self._qtlfit_call("binary", origin.shape[0], _p(origin), pheno, cov, use, perm, max_iter, tol,
                                 self._fit_flags(flags, additive, imprint), out)

    def qtl_scan_binary_device(self, n, d_origin, pheno, cov=None, imprint=False, use=None, perm=None, additive=False, max_iter=50,
                               tol=1e-7, out=None, flags=0):
        """The same on device rows, read in place (d_origin as for qtl_scan_device; None: the rows this context's last
        sweep_qtl left in it, which this call leaves valid).  With OUT_DEVICE in flags, out is a dict of device pointers."""
        return self._qtlfit_call("binary", n, C.c_void_p(d_origin), pheno, cov, use, perm, max_iter, tol,
                                 self._fit_flags(flags | QTL_ORIGIN_DEVICE, additive, imprint), out)

    # -- survival-trait single-locus scan: Cox regression ------------------------------
    def set_qtlsurv_columns(self, cap):
        """Cap on the columns per tile of qtl_scan_surv (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtlsurv_columns(self.h, cap), "cnf2_set_qtlsurv_columns")

    def set_qtlsurv_blocks(self, cap):
        """Cap on the blocks of qtl_scan_surv's launches (0 = the default); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtlsurv_blocks(self.h, cap), "cnf2_set_qtlsurv_blocks")

    def qtl_scan_surv(self, origin, time, status, cov=None, imprint=False, use=None, perm=None, additive=False, max_iter=50,
                      tol=1e-7, out=None, flags=0):
        """cnf2_qtl_scan_surv on host rows origin[n][M][4]: per marker Cox's proportional hazards regression of the columns
        (time[n][T], status[n][T]; 1 = event, 0 = censored) on the covariates cov[n][K] and the effects a, d (not with
        additive) and i (with imprint), by Newton's method from the null fit, for the individuals of use[n] and the
        permutations perm[P][n].  A dict: lod[T][M], coef[T][M][ne] (NaN for a dropped effect), iters[T][M], status[T][M]
        (0 = stopped by tol, 1 = by max_iter, 2 = breakdown), rank[M], ll0[T][C], n_events[T][C], n_used[C],
        perm_max[P][T][C] (None without permutations).  The model: include/cnf2hip.h; cnf2freq_amd/qtl.py reads the
        results."""
        origin = self._origin_rows(origin)
        return self._qtlfit_call("surv", origin.shape[0], _p(origin), time, cov, use, perm, max_iter, tol,
                                 self._fit_flags(flags, additive, imprint), out, status)

    def qtl_scan_surv_device(self, n, d_origin, time, status, cov=None, imprint=False, use=None, perm=None, additive=False,
                             max_iter=50, tol=1e-7, out=None, flags=0):
        """The same on device rows, read in place (d_origin as for qtl_scan_device; None: the rows this context's last
        sweep_qtl left in it, which this call leaves valid).  With OUT_DEVICE in flags, out is a dict of device pointers."""
        return self._qtlfit_call("surv", n, C.c_void_p(d_origin), time, cov, use, perm, max_iter, tol,
                                 self._fit_flags(flags | QTL_ORIGIN_DEVICE, additive, imprint), out, status)

    # -- variance-QTL single-locus scan: mean and log-variance effects ------------------
    def set_qtlvar_columns(self, cap):
        """Cap on the columns per tile of qtl_scan_var (0 = what memory allows); results do not depend on it."""
        self._chk(self.L.cnf2_set_qtlvar_columns(self.h, cap), "cnf2_set_qtlvar_columns")

    def qtl_scan_var(self, origin, pheno, cov=None, n_var=0, imprint=False, use=None, perm=None, additive=False, max_iter=50,
                     tol=1e-7, out=None, flags=0):
        """cnf2_qtl_scan_var on host rows origin[n][M][4]: per marker the double generalised linear model of pheno[n][T] --
        the mean on the covariates cov[n][K], the log variance on the first n_var of them, both on the effects a, d (not with
        additive) and i (with imprint) -- fitted mean-only, variance-only and in full from the null fit, for the individuals
        of use[n] and the permutations perm[P][n].  A dict: lod[T][M][3] (joint, mean, variance), coef_mean and
        coef_var[T][M][ne] of the full fit (NaN for a dropped effect), iters and status[T][M][3] by fit (0 = stopped by tol,
        1 = by max_iter, 2 = breakdown), rank[M], ll0[T][C], n_used[C], perm_max[P][T][C][3] (None without permutations).
        The model: include/cnf2hip.h; cnf2freq_amd/qtl.py reads the results."""
        origin = self._origin_rows(origin)
        return self._qtlfit_call("var", origin.shape[0], _p(origin), pheno, cov, use, perm, max_iter, tol,
                                 self._fit_flags(flags, additive, imprint), out, n_var)

    def qtl_scan_var_device(self, n, d_origin, pheno, cov=None, n_var=0, imprint=False, use=None, perm=None, additive=False,
                            max_iter=50, tol=1e-7, out=None, flags=0):
        """The same on device rows, read in place (d_origin as for qtl_scan_device; None: the rows this context's last
        sweep_qtl left in it, which this call leaves valid).  With OUT_DEVICE in flags, out is a dict of device pointers."""
        return self._qtlfit_call("var", n, C.c_void_p(d_origin), pheno, cov, use, perm, max_iter, tol,
                                 self._fit_flags(flags | QTL_ORIGIN_DEVICE, additive, imprint), out, n_var)

    def turn_scan_rows(self, ind, chrom=0):
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros((mc, 128, 8))
        self._chk(self.L.cnf2_turn_scan_rows(self.h, ind, chrom, _p(v)), "cnf2_turn_scan_rows")
        return v

    def haplos(self, ind, chrom=0, ties=True):
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros((mc, 7, 2))
        self._chk(self.L.cnf2_haplos(self.h, ind, chrom, _p(v), 0 if ties else NO_TIES), "cnf2_haplos")
        return v

    def infprobs(self, ind, marker, chrom=0, ties=True):
        inf = np.zeros((7, 2, 2))
        hz = np.zeros(2)
        self._chk(self.L.cnf2_infprobs(self.h, ind, chrom, marker, _p(inf), _p(hz), 0 if ties else NO_TIES),
                  "cnf2_infprobs")
        return inf, hz

    def infprobs_rows(self, ind, chrom=0, ties=True):
        """Closed-form rows for every marker of the chromosome: (inf[mc][7][2][2], hz[mc][2])."""
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros((mc, 30))
        self._chk(self.L.cnf2_infprobs_rows(self.h, ind, chrom, _p(v), 0 if ties else NO_TIES), "cnf2_infprobs_rows")
        return v[:, :28].reshape(mc, 7, 2, 2).copy(), v[:, 28:].copy()

    def descendants(self):
        d = np.zeros(self.n_rec, np.int32)
        self._chk(self.L.cnf2_descendants(self.h, _p(d)), "cnf2_descendants")
        return d

    def accumulate(self, desc, ind_begin=0, ind_end=None, ties=True):
        ind_end = self.n_ind if ind_end is None else ind_end
        desc = np.ascontiguousarray(desc, np.int32)
        inf = np.zeros((self.n_rec, self.n_markers, 2, 2))
        hb = np.zeros((self.n_rec, self.n_markers))
        hc = np.zeros((self.n_rec, self.n_markers))
        hz = np.zeros((ind_end - ind_begin, self.n_markers, 2))
        self._chk(self.L.cnf2_accumulate(self.h, ind_begin, ind_end, _p(desc), _p(inf), _p(hb), _p(hc), _p(hz),
                                         0 if ties else NO_TIES), "cnf2_accumulate")
        return dict(infprobs=inf, haplobase=hb, haplocount=hc, homozyg=hz)

    def sweep_accumulate(self, desc, ind_begin=0, ind_end=None, ties=True, raw=False, table_form=False, lane_form=False,
                         ties_general=False, deterministic=False, static_jobs=False, rows=True, all_states=False):
        """One haplotyping sweep: the outputs of sweep() and the per-record accumulators, batched on the device.
        rows=False: no dosage pointer is passed (what an iteration that prints no rows does): "dosage" comes back as zeros."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        desc = np.ascontiguousarray(desc, np.int32)
        factors = np.zeros((n, self.n_chrom, 8))
        loglik = np.zeros((n, self.n_chrom))
        dos = np.zeros((n, self.n_markers, 3))
        inf = np.zeros((self.n_rec, self.n_markers, 2, 2))
        hb = np.zeros((self.n_rec, self.n_markers))
        hc = np.zeros((self.n_rec, self.n_markers))
        hz = np.zeros((n, self.n_markers, 2))
        self._chk(self.L.cnf2_sweep_accumulate(self.h, ind_begin, ind_end, _p(desc), _p(factors), _p(loglik), _p(dos) if rows else None,
                                               _p(inf), _p(hb), _p(hc), _p(hz),
                                               (0 if ties else NO_TIES) | (RAW_DOSAGE if raw else 0)
                                               | (ACC_TABLE if table_form else 0) | (ACC_LANES if lane_form else 0)
                                               | (TIES_GENERAL if ties_general else 0)
                                               | (DETERMINISTIC if deterministic else 0) | (STATIC_JOBS if static_jobs else 0) | (ALL_STATES if all_states else 0)),
                  "cnf2_sweep_accumulate")
        return dict(factors=factors, loglik=loglik, dosage=dos, infprobs=inf, haplobase=hb, haplocount=hc, homozyg=hz)

    def sweep_accumulate_device(self, desc, ind_begin, ind_end, d_factors, d_loglik, d_dosage, d_inf, d_hb, d_hc, d_hz,
                                flags=0):
        """Device-pointer form (ints): outputs and accumulators stay on the GPU; only enqueues (use sync())."""
        desc = np.ascontiguousarray(desc, np.int32)
        self._chk(self.L.cnf2_sweep_accumulate(self.h, ind_begin, ind_end, _p(desc), C.c_void_p(d_factors),
                                               C.c_void_p(d_loglik), C.c_void_p(d_dosage), C.c_void_p(d_inf),
                                               C.c_void_p(d_hb), C.c_void_p(d_hc), C.c_void_p(d_hz),
                                               flags | OUT_DEVICE | ACC_DEVICE), "cnf2_sweep_accumulate")

    def sweep_turn_scan(self, ind_begin=0, ind_end=None, full=True, lse=True, ties=True, ties_general=False, valu=False,
                        static_jobs=False, all_states=False):
        """Batched turn scan: rawervals [n][M][128][8] and / or their log-sum-exp over the admissible modes [n][M][128]."""
        ind_end = self.n_ind if ind_end is None else ind_end
        n = ind_end - ind_begin
        raw = np.zeros((n, self.n_markers, 128, 8)) if full else None
        ls = np.zeros((n, self.n_markers, 128)) if lse else None
        self._chk(self.L.cnf2_sweep_turn_scan(self.h, ind_begin, ind_end, _p(raw) if full else None, _p(ls) if lse else None,
                                              (0 if ties else NO_TIES) | (TIES_GENERAL if ties_general else 0)
                                              | (TURN_VALU if valu else 0) | (STATIC_JOBS if static_jobs else 0) | (ALL_STATES if all_states else 0)),
                  "cnf2_sweep_turn_scan")
        return raw, ls

    def fixparents_scan(self, recs):
        recs = np.ascontiguousarray(recs, np.int32)
        ok = np.zeros((len(recs), self.n_markers, 2), np.uint8)
        self._chk(self.L.cnf2_fixparents_scan(self.h, _p(recs), len(recs), _p(ok)), "cnf2_fixparents_scan")
        return ok

    def variances(self, recs, ordered=True, brute=False):
        recs = np.ascontiguousarray(recs, np.int32)
        v = np.zeros((len(recs), self.n_markers))
        self._chk(self.L.cnf2_variances(self.h, _p(recs), len(recs), (1 if ordered else 0) | (2 if brute else 0), _p(v)),
                  "cnf2_variances")
        return v

    def variances_exact(self, recs, markers, ordered=True):
        """addvariance of (recs[q], markers[q]) with the reference's own rounding (cnf2_variances_exact)"""
        recs, markers = np.ascontiguousarray(recs, np.int32), np.ascontiguousarray(markers, np.int32)
        assert recs.shape == markers.shape
        v = np.zeros(len(recs))
        self._chk(self.L.cnf2_variances_exact(self.h, _p(recs), _p(markers), len(recs), 1 if ordered else 0, _p(v)), "cnf2_variances_exact")
        return v

    def snapshot_priors(self, has_prior):
        hp = np.ascontiguousarray(has_prior, np.uint8)
        assert len(hp) == self.n_rec
        self._chk(self.L.cnf2_snapshot_priors(self.h, _p(hp)), "cnf2_snapshot_priors")

    def update_pass(self, chrom, children, descendants, scalefactor, entropyfactor=1.0, acc=None, flags=0):
        """acc: dict with host arrays infprobs / haplobase / haplocount (updated in place), or None for the
        accumulators the last sweep_accumulate(..., keep=True) left in the context.  Returns hitnnn."""
        ch = np.ascontiguousarray(children, np.int32)
        de = np.ascontiguousarray(descendants, np.int32)
        hits = np.zeros(1, np.int32)
        a = (None, None, None) if acc is None else (_p(acc["infprobs"]), _p(acc["haplobase"]), _p(acc["haplocount"]))
        self._chk(self.L.cnf2_update_pass(self.h, chrom, _p(ch), _p(de), a[0], a[1], a[2], scalefactor, entropyfactor,
                                          _p(hits), flags), "cnf2_update_pass")
        return int(hits[0])

    def update_pass_records(self, chrom, recs, children, descendants, scalefactor, entropyfactor=1.0, flags=0):
        """update_pass restricted to the listed records (ascending), on the accumulators the context holds."""
        rc_ = np.ascontiguousarray(recs, np.int32)
        ch = np.ascontiguousarray(children, np.int32)
        de = np.ascontiguousarray(descendants, np.int32)
        hits = np.zeros(1, np.int32)
        self._chk(self.L.cnf2_update_pass_records(self.h, chrom, _p(rc_), len(rc_), _p(ch), _p(de), scalefactor, entropyfactor,
                                                  _p(hits), flags), "cnf2_update_pass_records")
        return int(hits[0])

    def window_table(self):
        """window_info() of every analysed individual in one call: int32 [n_ind][17]."""
        out = np.zeros((self.n_ind, 17), np.int32)
        self._chk(self.L.cnf2_window_table(self.h, _p(out)), "cnf2_window_table")
        return out

    def exchange_buffer(self, nbytes):
        p = C.c_void_p(0)
        self._chk(self.L.cnf2_exchange_buffer(self.h, nbytes, C.byref(p)), "cnf2_exchange_buffer")
        return p.value

    def pack_accumulators(self, recs, d_packed):
        r = np.ascontiguousarray(recs, np.int32)
        self._chk(self.L.cnf2_pack_accumulators(self.h, _p(r), len(r), C.c_void_p(d_packed)), "cnf2_pack_accumulators")

    def unpack_accumulators(self, recs, d_packed):
        r = np.ascontiguousarray(recs, np.int32)
        self._chk(self.L.cnf2_unpack_accumulators(self.h, _p(r), len(r), C.c_void_p(d_packed)), "cnf2_unpack_accumulators")

    def pack_rows(self, recs, d_packed):
        r = np.ascontiguousarray(recs, np.int32)
        self._chk(self.L.cnf2_pack_rows(self.h, _p(r), len(r), C.c_void_p(d_packed)), "cnf2_pack_rows")

    def unpack_rows(self, recs, d_packed):
        r = np.ascontiguousarray(recs, np.int32)
        self._chk(self.L.cnf2_unpack_rows(self.h, _p(r), len(r), C.c_void_p(d_packed)), "cnf2_unpack_rows")

    def clock_probe(self):
        """Shader clock under a double-precision vector load, MHz."""
        v = C.c_double(0)
        self._chk(self.L.cnf2_clock_probe(self.h, C.byref(v)), "cnf2_clock_probe")
        return v.value

    def sweep_clock(self):
        """Shader clock of the last sweep's untied fast-kernel launch (its own counters), MHz; 0 if none ran."""
        v = C.c_double(0)
        self._chk(self.L.cnf2_sweep_clock(self.h, C.byref(v)), "cnf2_sweep_clock")
        return v.value

    def update_stats(self):
        """Diagnostics of the last update pass: dict of (flows, steps, slots, refills) for certainty / haploweight."""
        out = np.zeros(16, np.uint64)
        self._chk(self.L.cnf2_update_stats(self.h, _p(out)), "cnf2_update_stats")
        names = ("flows", "scout_evaluations", "ended_in_scout", "pinned", "finish_steps", "finish_slots", "quadratures", "ended_by_tolerance")
        return dict(certainty=dict(zip(names, (int(x) for x in np.r_[out[0:4], out[8:12]]))),
                    haploweight=dict(zip(names, (int(x) for x in np.r_[out[4:8], out[12:16]]))))

    def download_accumulators(self):
        """The accumulators the context holds: dict(infprobs [R][M][2][2], haplobase [R][M], haplocount [R][M])."""
        R, M = self.n_rec, self.n_markers
        inf, hb, hc = np.zeros((R, M, 2, 2)), np.zeros((R, M)), np.zeros((R, M))
        self._chk(self.L.cnf2_download_accumulators(self.h, _p(inf), _p(hb), _p(hc)), "cnf2_download_accumulators")
        return dict(infprobs=inf, haplobase=hb, haplocount=hc)

    @staticmethod
    def accumulators_of(ctx_handle, n_rec, n_markers):
        """download_accumulators() for a raw cnf2_ctx handle (e.g. cnf2h_context of a host run)."""
        L = load()
        inf, hb, hc = np.zeros((n_rec, n_markers, 2, 2)), np.zeros((n_rec, n_markers)), np.zeros((n_rec, n_markers))
        if L.cnf2_download_accumulators(ctx_handle, _p(inf), _p(hb), _p(hc)) != 0:
            raise Cnf2Error("cnf2_download_accumulators: " + L.cnf2_last_error(ctx_handle).decode())
        return dict(infprobs=inf, haplobase=hb, haplocount=hc)

    def upload_accumulators(self, acc):
        a = [np.ascontiguousarray(acc[k], np.float64) for k in ("infprobs", "haplobase", "haplocount")]
        self._chk(self.L.cnf2_upload_accumulators(self.h, _p(a[0]), _p(a[1]), _p(a[2])), "cnf2_upload_accumulators")

    def download_rows(self, row0, n):
        allele = np.zeros((n, self.n_markers, 2), np.uint8)
        sure = np.zeros((n, self.n_markers, 2))
        hw = np.zeros((n, self.n_markers))
        self._chk(self.L.cnf2_download_rows(self.h, row0, n, _p(allele), _p(sure), _p(hw)), "cnf2_download_rows")
        return allele, sure, hw

    def addvariance(self, ind, chrom=0):
        mc = int(self.chromstarts[chrom + 1] - self.chromstarts[chrom])
        v = np.zeros(mc)
        self._chk(self.L.cnf2_addvariance(self.h, ind, chrom, _p(v)), "cnf2_addvariance")
        return v

    def emission(self, ind, marker):
        e = np.zeros((8, 64))
        self._chk(self.L.cnf2_emission(self.h, ind, marker, _p(e)), "cnf2_emission")
        return e

    def emission_paths(self, ind, marker):
        e = np.zeros((8, 64, 128))
        self._chk(self.L.cnf2_emission_paths(self.h, ind, marker, _p(e)), "cnf2_emission_paths")
        return e

    def selftest_lane_xor(self):
        out = np.zeros((6, 64))
        self._chk(self.L.cnf2_selftest_lane_xor(self.h, _p(out)), "cnf2_selftest_lane_xor")
        return out
