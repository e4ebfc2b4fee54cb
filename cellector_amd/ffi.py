"""ctypes binding of libcellector_hip.so (include/cellector_ffi.h).

Host-side plumbing only: every computation happens in the HIP library.  There is no CPU fallback — if the
library is missing or no GPU is present, construction fails loudly.
"""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CELLECTOR_HIP_LIB") or os.path.join(_HERE, "libcellector_hip.so")

XCHG_PASS1, XCHG_NORM, XCHG_LOCUS = 0, 1, 2
K_CELL_LL, K_LOCUS_STATS, K_SELECT, K_POSTERIOR, K_TILE_LL, K_CELL_VAR, K_LOCUS_MOM = 0, 1, 2, 3, 4, 5, 6
STATUS_NAMES = {0: "OK", 1: "EINVAL", 2: "EIO", 3: "EPARSE", 4: "ENOMEM", 5: "EDEVICE", 6: "ECOMM"}

# every entry point include/cellector_ffi.h declares: name -> (restype, argtypes)
_vp, _u64, _d, _cp, _i = C.c_void_p, C.c_uint64, C.c_double, C.c_char_p, C.c_int
SIGNATURES = {
    "cellector_create": (_i, [C.POINTER(_vp), _i]),
    "cellector_destroy": (None, [_vp]),
    "cellector_device_count": (_i, [C.POINTER(_i)]),
    "cellector_create_multi": (_i, [C.POINTER(_vp), C.POINTER(_i), _i]),
    "cellector_comm_unique_id": (_i, [_vp]),
    "cellector_comm_init_rank": (_i, [_vp, _vp, _i, _i]),
    "cellector_last_error": (_cp, [_vp]),
    "cellector_version": (_cp, []),
    "cellector_set_stream": (_i, [_vp, _vp]),
    "cellector_set_option": (_i, [_vp, _cp, C.c_int64]),
    "cellector_set_shard": (_i, [_vp, _u64, _u64]),
    "cellector_set_partition": (_i, [_vp, _vp, _i]),
    "cellector_partition": (_i, [_vp, _vp, C.POINTER(_i)]),
    "cellector_ingest_mtx": (_i, [_vp, _cp, _cp]),
    "cellector_ingest_coo": (_i, [_vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp]),
    "cellector_ingest_synthetic": (_i, [_vp, _u64, _u64, _d, _u64, _d, _d]),
    "cellector_write_staged_mtx": (_i, [_vp, C.c_char_p, C.c_char_p]),
    "cellector_ingest_finish": (_i, [_vp, _u64, _u64]),
    "cellector_load_mtx": (_i, [_vp, _cp, _cp, _u64, _u64]),
    "cellector_load_coo": (_i, [_vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _u64]),
    "cellector_ingest_mtx_joined": (_i, [_vp, _cp, _cp, _i, _vp]),
    "cellector_load_mtx_joined": (_i, [_vp, _cp, _cp, _i, _u64, _u64, _vp]),
    "cellector_ingest_coo_joined": (_i, [_vp, _u64, _u64, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _i, _vp]),
    "cellector_dims": (_i, [_vp, _vp]),
    "cellector_locus_ids": (_i, [_vp, _vp]),
    "cellector_locus_counts": (_i, [_vp, _vp]),
    "cellector_entries_per_cell": (_i, [_vp, _vp]),
    "cellector_csr_rows": (_i, [_vp, _u64, _u64, _vp, _vp, _u64]),
    "cellector_restage": (_i, [_vp, _vp, _d, _u64]),
    "cellector_cell_origin": (_i, [_vp, _vp]),
    "cellector_staged_coo": (_i, [_vp, C.POINTER(_u64), _vp, _vp, _vp, _vp, _u64]),
    "cellector_combine": (_i, [_vp, _vp, _vp, _vp, _u64, _d, _u64]),
    "cellector_cell_source": (_i, [_vp, _vp]),
    "cellector_add_doublets": (_i, [_vp, _vp, _vp, _u64, _d, _u64]),
    "cellector_write_mtx": (_i, [_vp, _cp, _cp, _i, C.c_uint32, _vp]),
    "cellector_format_mtx": (_i, [_vp, _i, _i, C.c_uint32, _u64, _u64, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "cellector_bgzf_compress": (_i, [_vp, _vp, _u64, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "cellector_write_mtx_bgzf": (_i, [_vp, _cp, _cp, _i, C.c_uint32, _vp]),
    "cellector_bgzf_decompress": (_i, [_vp, _vp, _u64, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "cellector_exchange_buffer": (_i, [_vp, _i, C.POINTER(_vp), C.POINTER(_u64)]),
    "cellector_bind_exchange_buffer": (_i, [_vp, _i, _vp, _u64]),
    "cellector_em_begin": (_i, [_vp]),
    "cellector_em_threshold": (_i, [_vp, _d]),
    "cellector_em_finish": (_i, [_vp, _vp]),
    "cellector_em_iteration": (_i, [_vp, _d, _vp]),
    "cellector_set_excluded": (_i, [_vp, _vp]),
    "cellector_set_loci_mask": (_i, [_vp, _vp]),
    "cellector_em_reset": (_i, [_vp]),
    "cellector_iter_resolution": (_i, [_vp, _vp]),
    "cellector_iter_resolved_cells": (_i, [_vp, _vp]),
    "cellector_iter_cell_outputs": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cellector_iter_locus_outputs": (_i, [_vp] + [_vp] * 8),
    "cellector_loci_mask": (_i, [_vp, _vp]),
    "cellector_excluded": (_i, [_vp, _vp]),
    "cellector_alpha_betas": (_i, [_vp, _vp, _vp]),
    "cellector_cell_log_likelihoods": (_i, [_vp] + [_vp] * 6),
    "cellector_cell_pmfs": (_i, [_vp, _vp, _vp, _vp, _vp, _u64, _vp, _u64] + [_vp] * 6),
    "cellector_cell_log_variances": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cellector_iter_cell_variances": (_i, [_vp, _vp]),
    "cellector_locus_moments": (_i, [_vp] + [_vp] * 8),
    "cellector_locus_total_counts": (_i, [_vp, _vp, _vp]),
    "cellector_iter_locus_moments": (_i, [_vp] + [_vp] * 4),
    "cellector_posterior_alpha_betas": (_i, [_vp, _i, _vp, _vp]),
    "cellector_posteriors": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cellector_class_tallies": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "cellector_class_alpha_betas": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "cellector_class_posteriors": (_i, [_vp, _vp, C.c_uint32] + [_vp] * 7),
    "cellector_refine_classes": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, C.c_uint32, _u64] + [_vp] * 4),
    "cellector_class_pair_alpha_betas": (_i, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp]),
    "cellector_class_doublets": (_i, [_vp, _vp, _vp, C.c_uint32] + [_vp] * 13),
    "cellector_refine_class_doublets": (_i, [_vp, _vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, C.c_double, C.c_uint32, _u64]
                                        + [_vp] * 7),
    "cellector_class_genotypes": (_i, [_vp, _vp, C.c_uint32, _d, _d] + [_vp] * 6),
    "cellector_cluster_default_params": (_i, [_vp]),
    "cellector_cluster": (_i, [_vp, C.c_uint32, C.c_uint32, _u64] + [_vp] * 8),
    "cellector_cluster_m_step": (_i, [_vp, _vp, C.c_uint32, _vp, _d] + [_vp] * 4),
    "cellector_cluster_e_step": (_i, [_vp, _vp, C.c_uint32, C.c_uint32] + [_vp] * 5),
    "cellector_donor_default_params": (_i, [_vp]),
    "cellector_donor_tables": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "cellector_donor_posteriors": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp] + [_vp] * 14),
    "cellector_match_donors": (_i, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp] + [_vp] * 4),
    "cellector_donor_panel": (_i, [_vp, _vp, C.c_uint32, C.c_uint32, _vp, _vp, _vp, _vp] + [_vp] * 19),
    "cellector_match_donors_panel": (_i, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp] + [_vp] * 4),
    "cellector_donor_fit_default_params": (_i, [_vp]),
    "cellector_donor_moment_tables": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cellector_donor_fit": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp] + [_vp] * 14),
    "cellector_donor_posteriors_gp": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp] + [_vp] * 14),
    "cellector_donor_weights": (_i, [_vp, _vp, C.c_uint32, _vp, _vp]),
    "cellector_match_donors_gp": (_i, [_vp, _vp, C.c_uint32, _vp, C.c_uint32, _vp, _vp] + [_vp] * 4),
    "cellector_ambient_default_params": (_i, [_vp]),
    "cellector_ambient_tables": (_i, [_vp, _vp, C.c_uint32, _d, _vp, _vp]),
    "cellector_ambient_profile": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, C.c_uint32, _d, _u64, _vp] + [_vp] * 8),
    "cellector_estimate_ambient": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp] + [_vp] * 4),
    "cellector_pair_fraction_default_params": (_i, [_vp]),
    "cellector_pair_fraction_tables": (_i, [_vp, _vp, _vp, C.c_uint32, _vp, _vp]),
    "cellector_donor_pair_fractions": (_i, [_vp, _vp, C.c_uint32, _vp, _vp, _vp, _vp, _vp, C.c_uint32, _vp] + [_vp] * 8),
    "cellector_donor_genotypes_default_params": (_i, [_vp]),
    "cellector_donor_genotypes": (_i, [_vp, _vp, _vp, C.c_uint32, _vp] + [_vp] * 9),
    "cellector_assign": (_i, [_vp, _d, _u64] + [_vp] * 7),
    "cellector_assign_resolution": (_i, [_vp, _vp]),
    "cellector_assign_resolved_cells": (_i, [_vp, _vp]),
    "cellector_final_allele_tallies": (_i, [_vp, _vp, _vp, _vp, _vp]),
    "cellector_engine_info": (_i, [_vp, _vp]),
    "cellector_order_statistics": (_i, [_vp, _vp, _u64, _d, _vp]),
    "cellector_kernel_time": (_i, [_vp, _i, C.POINTER(_d), C.POINTER(_u64)]),
    "cellector_reset_timing": (_i, [_vp]),
}


class Dims(C.Structure):
    _fields_ = [("total_cells", _u64), ("total_loci", _u64), ("loci_used", _u64), ("cell_begin", _u64),
                ("cell_end", _u64), ("nnz_used", _u64)]


class EngineInfo(C.Structure):
    _fields_ = [("engine", _u64), ("nnz_regular", _u64), ("nnz_overflow", _u64), ("tile_bytes", _u64),
                ("cell_blocks", _u64), ("locus_chunks", _u64), ("chunk_groups", _u64), ("tile_lookups", _u64)]


class IterSummary(C.Structure):
    _fields_ = [("any_change", C.c_int32), ("n_new_excluded", _u64), ("n_rescued", _u64), ("n_excluded", _u64),
                ("n_loci_filtered", _u64), ("median", _d), ("iqr", _d), ("threshold", _d), ("n_near_threshold", _u64)]


class Resolution(C.Structure):
    _fields_ = [("n_evaluated", _u64), ("n_flags_changed", _u64), ("changed", C.c_uint32), ("mode", C.c_uint32)]


class AssignResolution(C.Structure):
    _fields_ = [("n_evaluated", _u64), ("n_labels_changed", _u64), ("n_qual_changed", _u64), ("mode", C.c_uint32),
                ("reserved", C.c_uint32)]


class RefineSummary(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("converged", C.c_uint32), ("n_moved_last", _u64), ("n_moved_total", _u64),
                ("n_recounts", _u64), ("class_cells", _u64 * 16)]


class RefineDoubletsSummary(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("converged", C.c_uint32), ("n_moved_last", _u64), ("n_moved_total", _u64),
                ("n_recounts", _u64), ("class_cells", _u64 * 16), ("n_held", _u64)]


class ClusterParams(C.Structure):
    _fields_ = [("theta_floor", _d), ("anneal_base", _d), ("tol", _d), ("anneal_steps", C.c_uint32), ("max_iter", C.c_uint32),
                ("min_loci", _u64)]


class ClusterSummary(C.Structure):
    _fields_ = [("best_restart", C.c_uint32), ("iterations", C.c_uint32), ("stages", C.c_uint32), ("reserved", C.c_uint32),
                ("iterations_per_stage", C.c_uint32 * 16), ("cluster_cells", _u64 * 16), ("n_unlabelled", _u64)]


class DonorParams(C.Structure):
    _fields_ = [("err", _d), ("ambient", _d), ("doublet_rate", _d), ("posterior_threshold", _d), ("min_loci", _u64)]


class DonorSummary(C.Structure):
    _fields_ = [("n_singlet", _u64), ("n_doublet", _u64), ("n_ambiguous", _u64), ("n_unassigned", _u64), ("donor_cells", _u64 * 64)]


class DonorPanelSummary(C.Structure):
    _fields_ = [("n_singlet", _u64), ("n_doublet", _u64), ("n_ambiguous", _u64), ("n_unassigned", _u64), ("n_present", _u64)]


class DonorFitParams(C.Structure):
    _fields_ = [("iqr_multiple", _d), ("min_cells", _u64)]


class DonorFitSummary(C.Structure):
    _fields_ = [("n_keys", _u64), ("median", _d), ("iqr", _d), ("threshold", _d), ("n_unmatched", _u64), ("n_unmatched_singlet", _u64),
                ("n_unmatched_doublet", _u64), ("n_unmatched_ambiguous", _u64), ("donor_unmatched", _u64 * 64)]


class AmbientParams(C.Structure):
    _fields_ = [("err", _d), ("lo", _d), ("hi", _d), ("grid", C.c_uint32), ("rounds", C.c_uint32), ("min_loci", _u64)]


class AmbientSummary(C.Structure):
    _fields_ = [("rho", _d), ("se", _d), ("curvature", _d), ("log_likelihood", _d), ("lo", _d), ("hi", _d), ("j_star", C.c_uint32),
                ("at_boundary", C.c_uint32), ("rounds", C.c_uint32), ("reserved", C.c_uint32), ("n_cells_used", _u64),
                ("source_rho", _d * 64), ("source_se", _d * 64), ("source_cells", _u64 * 64)]


class PairFractionParams(C.Structure):
    _fields_ = [("min_fraction", _d), ("min_loci", _u64)]


class PairFractionSummary(C.Structure):
    _fields_ = [("n_balanced", _u64), ("n_toward_a", _u64), ("n_toward_b", _u64), ("n_flat", _u64), ("n_none", _u64),
                ("donor_cells", _u64 * 64)]


class DonorGenotypesParams(C.Structure):
    _fields_ = [("err", _d), ("ambient", _d), ("gt_threshold", _d), ("prior_floor", _d)]


class DonorGenotypesSummary(C.Structure):
    _fields_ = [("cells", _u64 * 64), ("loci_with_reads", _u64 * 64), ("confirmed", _u64 * 64), ("filled", _u64 * 64),
                ("changed", _u64 * 64), ("withdrawn", _u64 * 64)]

    def as_dict(self, n_donors):
        """the fields donor_genotypes.summary returns, cut to the D donors"""
        return {k: np.array(getattr(self, k)[:n_donors], np.uint64) for k, _ in self._fields_}


class JoinSummary(C.Structure):
    _fields_ = [("n_first", _u64), ("n_second", _u64), ("n_both", _u64), ("n_first_only", _u64), ("n_second_only", _u64), ("n_out", _u64),
                ("first_sorted", C.c_uint32), ("second_sorted", C.c_uint32), ("join_tile", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        """the fields join.join_coo returns as its summary"""
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class WriteSummary(C.Structure):
    _fields_ = [("n_entries", _u64), ("lines_first", _u64), ("lines_second", _u64), ("bytes_first", _u64), ("bytes_second", _u64),
                ("n_dropped_keys", _u64), ("n_windows", _u64)]

    def as_dict(self):
        """the fields mtx_write.summary returns"""
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class WriteBgzfSummary(C.Structure):
    _fields_ = [("text", WriteSummary), ("file_bytes_first", _u64), ("file_bytes_second", _u64), ("blocks_first", _u64),
                ("blocks_second", _u64), ("stored_blocks", _u64)]

    def as_dict(self):
        """text: the fields mtx_write.summary returns; the rest: the files as they are"""
        out = {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "text"}
        out["text"] = self.text.as_dict()
        return out


WRITE_MODES = {"aligned": 0, "sparse": 1, "depth": 2, 0: 0, 1: 1, 2: 2}
MTX_SPACE, MTX_HEADER_ZERO = 1, 2


def _mtx_flags(sep, header_zero):
    if sep not in ("\t", " ", b"\t", b" "):
        raise ValueError("sep is a tab or a space")
    return (MTX_SPACE if sep in (" ", b" ") else 0) | (MTX_HEADER_ZERO if header_zero else 0)


JOIN_MODES = {"join": 1, "ref": 1, "depth": 2, 1: 1, 2: 2}


class CellectorError(RuntimeError):
    def __init__(self, status, message):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


_lib = None


def load_library(path=LIB_PATH):
    """dlopen the HIP library and attach signatures (no GPU needed for this step)."""
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    # PyTorch-ROCm ships its own copy of the HIP runtime.  A process that uses both this library and torch.cuda must load
    # torch's copy FIRST (this library then binds to it by soname); the other order leaves two runtimes in the process and
    # torch.cuda fails to initialise ("No HIP GPUs are available").  CELLECTOR_NO_TORCH=1 skips this (torch-free hosts).
    if "torch" not in sys.modules and not os.environ.get("CELLECTOR_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    if not os.path.exists(path):
        raise FileNotFoundError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                                "(cellector_amd has no CPU fallback)")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    if path == LIB_PATH:
        _lib = lib
    return lib


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Cellector:
    """One shard of a (locus x cell) matrix on one GPU; mirrors the reference's main() flow."""

    def __init__(self, device=0, stream=None, devices=None):
        """devices=[d0, d1, ...]: ONE ctx over several GPUs (cellector_create_multi; a device listed twice = logical
        shards on that GPU); every method then works on the whole matrix, arrays in global cell order."""
        self._lib = load_library()
        h = C.c_void_p()
        if devices is not None and len(devices) > 1:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            st = self._lib.cellector_create_multi(C.byref(h), ids, len(devices))
        else:
            st = self._lib.cellector_create(C.byref(h), int(devices[0] if devices else device))
        if st != 0:
            raise CellectorError(st, "cellector_create failed (no MI355X visible? the HIP path is mandatory)")
        self.h = h
        if stream is not None:
            self._ck(self._lib.cellector_set_stream(self.h, C.c_void_p(stream)))

    def _ck(self, st):
        if st != 0:
            raise CellectorError(st, self._lib.cellector_last_error(self.h).decode(errors="replace"))

    def close(self):
        if getattr(self, "h", None):
            self._lib.cellector_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- configuration
    def set_option(self, key, value):
        self._ck(self._lib.cellector_set_option(self.h, key.encode(), int(value)))

    def set_stream(self, stream):
        """hipStream_t as an integer (e.g. torch.cuda.current_stream().cuda_stream); 0 / None = the null stream"""
        self._ck(self._lib.cellector_set_stream(self.h, C.c_void_p(stream or None)))

    def comm_init_rank(self, unique_id, n_ranks, rank):
        """attach an RCCL communicator (one process per GPU); unique_id = the 128 bytes of comm_unique_id() on rank 0"""
        buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
        self._ck(self._lib.cellector_comm_init_rank(self.h, buf, int(n_ranks), int(rank)))

    def set_shard(self, cell_begin, cell_end):
        self._ck(self._lib.cellector_set_shard(self.h, int(cell_begin), int(cell_end)))

    def set_partition(self, bounds):
        """cell ranges of the ranks of a ctx with a communicator: n_ranks + 1 boundaries (None: back to the default)"""
        if bounds is None:
            self._ck(self._lib.cellector_set_partition(self.h, None, 0))
            return
        b = np.ascontiguousarray(bounds, dtype=np.uint64)
        self._ck(self._lib.cellector_set_partition(self.h, _p(b), len(b)))

    def partition(self):
        """the cell ranges in use: array of n_ranks + 1 boundaries"""
        n = C.c_int(0)
        self._ck(self._lib.cellector_partition(self.h, None, C.byref(n)))
        out = np.zeros(n.value + 1, np.uint64)
        self._ck(self._lib.cellector_partition(self.h, _p(out), C.byref(n)))
        return out

    # ---- ingest
    def ingest_mtx(self, alt_path, ref_path):
        self._ck(self._lib.cellector_ingest_mtx(self.h, str(alt_path).encode(), str(ref_path).encode()))

    def ingest_coo(self, total_loci, total_cells, locus0, cell0, alt, ref):
        arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (locus0, cell0, alt, ref)]
        self._ck(self._lib.cellector_ingest_coo(self.h, total_loci, total_cells, len(arrs[0]), *[_p(a) for a in arrs]))

    def ingest_synthetic(self, total_loci, total_cells, density, seed=4, minority_fraction=0.05, doublet_fraction=0.0):
        self._ck(self._lib.cellector_ingest_synthetic(self.h, total_loci, total_cells, float(density), int(seed),
                                                      float(minority_fraction), float(doublet_fraction)))

    def ingest_finish(self, min_alt=4, min_ref=4):
        self._ck(self._lib.cellector_ingest_finish(self.h, int(min_alt), int(min_ref)))

    def write_staged_mtx(self, alt_path, ref_path):
        """Benchmark utility: the staged matrix as a vartrix-style text pair (needs option keep_coo=1)."""
        self._ck(self._lib.cellector_write_staged_mtx(self.h, str(alt_path).encode(), str(ref_path).encode()))

    def load_mtx(self, alt_path, ref_path, min_alt=4, min_ref=4):
        self._ck(self._lib.cellector_load_mtx(self.h, str(alt_path).encode(), str(ref_path).encode(), min_alt, min_ref))

    def load_coo(self, total_loci, total_cells, locus0, cell0, alt, ref, min_alt=4, min_ref=4):
        self.ingest_coo(total_loci, total_cells, locus0, cell0, alt, ref)
        self.ingest_finish(min_alt, min_ref)

    # ---- joined ingest: two count matrices keyed by (locus, cell); mode "ref" / 1 (SECOND = ref counts) or "depth" / 2 (alt + ref)
    def ingest_mtx_joined(self, first_path, second_path, mode="ref"):
        """Stage the join of two .mtx files that need not list the same keys in the same order (cellector_ingest_mtx_joined;
        join.join_coo is the bit-identical numpy twin).  Returns the JoinSummary."""
        s = JoinSummary()
        self._ck(self._lib.cellector_ingest_mtx_joined(self.h, str(first_path).encode(), str(second_path).encode(), int(JOIN_MODES.get(mode, mode)), C.byref(s)))
        return s

    def load_mtx_joined(self, first_path, second_path, mode="ref", min_alt=4, min_ref=4):
        s = JoinSummary()
        self._ck(self._lib.cellector_load_mtx_joined(self.h, str(first_path).encode(), str(second_path).encode(), int(JOIN_MODES.get(mode, mode)), min_alt,
                                                     min_ref, C.byref(s)))
        return s

    def ingest_coo_joined(self, total_loci, total_cells, first, second, mode="ref"):
        """first, second: (locus0, cell0, count) triples in any order, e.g. (m.row, m.col, m.data) of two scipy COO matrices"""
        arrs = [[np.ascontiguousarray(a, dtype=np.uint32).ravel() for a in t] for t in (first, second)]
        for t in arrs:
            if len(t) != 3 or not (t[0].shape == t[1].shape == t[2].shape):
                raise ValueError("ingest_coo_joined: a stream is three arrays of one length: (locus0, cell0, count)")
        s = JoinSummary()
        self._ck(self._lib.cellector_ingest_coo_joined(self.h, total_loci, total_cells, len(arrs[0][0]), *[_p(a) for a in arrs[0]],
                                                       len(arrs[1][0]), *[_p(a) for a in arrs[1]], int(JOIN_MODES.get(mode, mode)), C.byref(s)))
        return s

    def load_synthetic(self, total_loci, total_cells, density, seed=4, minority_fraction=0.05, doublet_fraction=0.0,
                       min_alt=4, min_ref=4):
        self.ingest_synthetic(total_loci, total_cells, density, seed, minority_fraction, doublet_fraction)
        self.ingest_finish(min_alt, min_ref)

    # ---- accessors
    def dims(self):
        d = Dims()
        self._ck(self._lib.cellector_dims(self.h, C.byref(d)))
        return d

    @property
    def n_local(self):
        d = self.dims()
        return d.cell_end - d.cell_begin

    def locus_ids(self):
        out = np.empty(self.dims().loci_used, np.uint64)
        self._ck(self._lib.cellector_locus_ids(self.h, _p(out)))
        return out

    def locus_counts(self):
        out = np.empty((self.dims().loci_used, 2), np.float64)
        self._ck(self._lib.cellector_locus_counts(self.h, _p(out)))
        return out

    def entries_per_cell(self):
        out = np.empty(self.n_local, np.uint32)
        self._ck(self._lib.cellector_entries_per_cell(self.h, _p(out)))
        return out

    def csr_rows(self, row_begin, row_end):
        rp = np.empty(row_end - row_begin + 1, np.uint64)
        self._ck(self._lib.cellector_csr_rows(self.h, row_begin, row_end, _p(rp), None, 0))
        ent = np.empty(int(rp[-1]), np.uint64)
        self._ck(self._lib.cellector_csr_rows(self.h, row_begin, row_end, _p(rp), _p(ent), len(ent)))
        return rp, ent

    # ---- re-staging the resident matrix (cell subset, per-read downsampling) without the files
    def restage(self, keep=None, downsample_rate=0.0, seed=4):
        """A new staged matrix from the one the ctx holds (cellector_restage): the cells with keep != 0 (None: all), renumbered
        in ascending order, every read removed with probability downsample_rate (the combiner's meaning; restage.restage_coo is
        the bit-identical numpy twin).  The ctx is then STAGED: call ingest_finish(min_alt, min_ref) next.  A peel is three calls:
        c.restage(keep=c.excluded() == 0); c.ingest_finish(); c.run()."""
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
            n = self.dims().total_cells
            if keep.shape != (n,):
                raise ValueError(f"restage: {n} keep flags expected, got shape {keep.shape}")
        self._ck(self._lib.cellector_restage(self.h, _p(keep), float(downsample_rate), int(seed)))

    def cell_origin(self):
        """per current cell its index in the matrix of the last ingest from outside (cellector_cell_origin); identity until a
        restage drops cells, composed over repeated restages"""
        out = np.zeros(self.dims().total_cells, np.uint32)
        self._ck(self._lib.cellector_cell_origin(self.h, _p(out)))
        return out

    def staged_coo(self):
        """(locus0, cell0, alt, ref) uint32 arrays of the staged entries in staged order (cellector_staged_coo; diagnostic)"""
        n = C.c_uint64(0)
        self._ck(self._lib.cellector_staged_coo(self.h, C.byref(n), None, None, None, None, 0))
        arrs = [np.zeros(n.value, np.uint32) for _ in range(4)]
        if n.value:
            self._ck(self._lib.cellector_staged_coo(self.h, C.byref(n), *[_p(a) for a in arrs], n.value))
        return tuple(arrs)

    # ---- the staged matrix as mtx text, formatted on the GPU
    def write_mtx(self, first, second, mode="aligned", sep="\t", header_zero=False):
        """The staged matrix as a MatrixMarket text pair (cellector_write_mtx; mtx_write.write_pair is the byte-identical numpy
        twin).  mode "aligned": alt / ref with explicit zeros, one line per entry, what load_mtx reads and the combiner writes (with
        header_zero=True, its bytes); "sparse": the zero lines dropped, what load_mtx_joined(..., "ref") reads; "depth": alt and
        alt + ref, what load_mtx_joined(..., "depth") reads.  Only reads the ctx.  Returns the WriteSummary."""
        s = WriteSummary()
        self._ck(self._lib.cellector_write_mtx(self.h, str(first).encode(), str(second).encode(), int(WRITE_MODES.get(mode, mode)),
                                               _mtx_flags(sep, header_zero), C.byref(s)))
        return s

    def format_mtx(self, which, mode="aligned", first_entry=0, n_entries=None, sep="\t"):
        """the body lines of the staged entries [first_entry, first_entry + n_entries) of file `which` (0 / 1) as bytes
        (cellector_format_mtx); n_entries None: to the last entry"""
        if n_entries is None:
            n = C.c_uint64(0)
            self._ck(self._lib.cellector_staged_coo(self.h, C.byref(n), None, None, None, None, 0))
            n_entries = max(0, n.value - int(first_entry))
        m, fl = int(WRITE_MODES.get(mode, mode)), _mtx_flags(sep, False)
        nb, nl = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.cellector_format_mtx(self.h, int(which), m, fl, int(first_entry), int(n_entries), None, 0, C.byref(nb), C.byref(nl)))
        out = np.empty(nb.value, np.uint8)
        if nb.value:
            self._ck(self._lib.cellector_format_mtx(self.h, int(which), m, fl, int(first_entry), int(n_entries), _p(out), nb.value, C.byref(nb), C.byref(nl)))
        return out.tobytes()

    # ---- ... and as .mtx.gz: BGZF made on the GPU
    def write_mtx_bgzf(self, first, second, mode="aligned", sep="\t", header_zero=False):
        """write_mtx's pair as BGZF files (cellector_write_mtx_bgzf): each file is bgzf.compress of the file write_mtx writes with
        the same arguments, whatever option write_window says; load_mtx and load_mtx_joined read the paths as they are.  Returns
        the WriteBgzfSummary (its .text is write_mtx's summary)."""
        s = WriteBgzfSummary()
        self._ck(self._lib.cellector_write_mtx_bgzf(self.h, str(first).encode(), str(second).encode(), int(WRITE_MODES.get(mode, mode)),
                                                    _mtx_flags(sep, header_zero), C.byref(s)))
        return s

    def bgzf_compress(self, data):
        """`data` (bytes) as a BGZF stream, compressed on this ctx's GPU (cellector_bgzf_compress; bgzf.compress is the
        byte-identical numpy twin).  Works in any state of the ctx and leaves it as it is."""
        src = np.frombuffer(bytes(data), np.uint8)
        n_out, n_blocks = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.cellector_bgzf_compress(self.h, _p(src) if len(src) else None, len(src), None, 0, C.byref(n_out), C.byref(n_blocks)))
        out = np.empty(n_out.value, np.uint8)
        self._ck(self._lib.cellector_bgzf_compress(self.h, _p(src) if len(src) else None, len(src), _p(out), n_out.value, C.byref(n_out),
                                                   C.byref(n_blocks)))
        return out.tobytes()

    def bgzf_decompress(self, data):
        """The text of a BGZF stream `data` (bytes), inflated on this ctx's GPU (cellector_bgzf_decompress): what gzip.decompress
        returns, for bgzip's streams and this library's alike.  Works in any state of the ctx and leaves it as it is."""
        src = np.frombuffer(bytes(data), np.uint8)
        n_out, n_blocks = C.c_uint64(0), C.c_uint64(0)
        self._ck(self._lib.cellector_bgzf_decompress(self.h, _p(src) if len(src) else None, len(src), None, 0, C.byref(n_out), C.byref(n_blocks)))
        out = np.empty(n_out.value, np.uint8)
        self._ck(self._lib.cellector_bgzf_decompress(self.h, _p(src) if len(src) else None, len(src), _p(out) if n_out.value else _p(np.empty(1, np.uint8)),
                                                     n_out.value, C.byref(n_out), C.byref(n_blocks)))
        return out.tobytes()

    # ---- merging a second staged matrix in (the other half of the reference's combiner)
    def combine(self, src, keep=None, locus_map=None, total_loci=None, downsample_rate=0.0, seed=4):
        """The staged entries of `src` (another Cellector on the same GPU; only read) join this ctx's (cellector_combine): src's
        cells with keep != 0 (None: all) behind this ctx's cells, src's loci through locus_map (None: identity), src's reads
        thinned with downsample_rate; everything then ascends by (locus, cell, ref, alt) (combine.combine_coo is the
        bit-identical numpy twin).  total_loci defaults to the larger of this ctx's total_loci and src's (no map) or
        1 + locus_map.max() (with one).  The ctx is then STAGED: call ingest_finish(min_alt, min_ref) next.  A titration point:
        c.combine(minority, keep); c.ingest_finish(); c.run(); c.restage(keep=c.cell_source() == 0)."""
        sd = src.dims()
        if keep is not None:
            keep = np.ascontiguousarray(np.asarray(keep) != 0, dtype=np.uint8)
            if keep.shape != (sd.total_cells,):
                raise ValueError(f"combine: {sd.total_cells} keep flags expected, got shape {keep.shape}")
        if locus_map is not None:
            locus_map = np.ascontiguousarray(locus_map, dtype=np.uint32)
            if locus_map.shape != (sd.total_loci,):
                raise ValueError(f"combine: {sd.total_loci} map values expected, got shape {locus_map.shape}")
        if total_loci is None:
            theirs = sd.total_loci if locus_map is None else (1 + int(locus_map.max()) if locus_map.size else 0)
            total_loci = max(self.dims().total_loci, theirs)
        self._ck(self._lib.cellector_combine(self.h, src.h, _p(keep), _p(locus_map), int(total_loci), float(downsample_rate), int(seed)))

    def cell_source(self):
        """per current cell 0 = from the last ingest from outside, k = brought in by the k-th combine since
        (cellector_cell_source); restages compose it like cell_origin"""
        out = np.zeros(self.dims().total_cells, np.uint8)
        self._ck(self._lib.cellector_cell_source(self.h, _p(out)))
        return out

    # ---- synthetic doublets from resident cells
    def add_doublets(self, cell_a, cell_b, downsample_rate=0.0, seed=4):
        """One new cell per pair behind the ctx's cells (cellector_add_doublets): at every locus either parent covers it holds the
        sum of the counts of cell_a[j] and cell_b[j], every parent read removed on its way with probability downsample_rate,
        independently per (pair, side); the parents stay as they are and everything then ascends by (locus, cell, ref, alt)
        (doublets.add_doublets_coo is the bit-identical numpy twin).  The call counts as a combine: the new cells' cell_source()
        is the next number, their cell_origin() that of cell_a[j].  The ctx is then STAGED: call ingest_finish(min_alt, min_ref)
        next.  c.add_doublets(a, b, 0.5); c.ingest_finish(); c.run(); ...; c.restage(keep=c.cell_source() != k) takes them out."""
        pair = []
        for name, v in (("cell_a", cell_a), ("cell_b", cell_b)):
            v = np.asarray(v)
            if v.ndim != 1 or (v.size and v.dtype.kind not in "iu"):
                raise ValueError(f"add_doublets: {name} is not a list of cell indices")
            v = v.astype(np.int64) if v.dtype != np.uint64 else v
            if v.size and (int(v.min()) < 0 or int(v.max()) > 0xFFFFFFFF):
                raise ValueError(f"add_doublets: {name} holds an index outside 32 bits")
            pair.append(np.ascontiguousarray(v, dtype=np.uint32))
        if pair[0].shape != pair[1].shape:
            raise ValueError(f"add_doublets: {pair[0].size} cells a, {pair[1].size} cells b")
        self._ck(self._lib.cellector_add_doublets(self.h, _p(pair[0]), _p(pair[1]), pair[0].size, float(downsample_rate), int(seed)))

    def exchange_buffer(self, which):
        ptr, n = C.c_void_p(), C.c_uint64()
        self._ck(self._lib.cellector_exchange_buffer(self.h, which, C.byref(ptr), C.byref(n)))
        return ptr.value, n.value

    def bind_exchange_buffer(self, which, dev_ptr, n_f64):
        self._ck(self._lib.cellector_bind_exchange_buffer(self.h, which, C.c_void_p(dev_ptr), int(n_f64)))

    # ---- EM loop
    def em_begin(self):
        self._ck(self._lib.cellector_em_begin(self.h))

    def em_threshold(self, iqr_multiple=5.0):
        self._ck(self._lib.cellector_em_threshold(self.h, float(iqr_multiple)))

    def em_finish(self):
        s = IterSummary()
        self._ck(self._lib.cellector_em_finish(self.h, C.byref(s)))
        return s

    def em_iteration(self, iqr_multiple=5.0):
        s = IterSummary()
        self._ck(self._lib.cellector_em_iteration(self.h, float(iqr_multiple), C.byref(s)))
        return s

    def run(self, iqr_multiple=5.0, max_iter=1000):
        """cellector() outer loop (main.rs:42-46)."""
        out = []
        for _ in range(max_iter):
            s = self.em_iteration(iqr_multiple)
            out.append(s)
            if not s.any_change:
                break
        return out

    # ---- placing the EM state (exclusion set, loci mask) without a reload
    def set_excluded(self, flags):
        """excluded_cells := {i : flags[i] != 0} (cellector_set_excluded): local cells, or all cells of a multi-device ctx.
        The ctx is then the one whose last iteration produced this set: alpha_betas(), posteriors(), assign(),
        final_allele_tallies() use it, the next em_iteration() counts new / rescued cells against it."""
        f = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8)
        if f.shape != (self.n_local,):
            raise ValueError(f"set_excluded: {self.n_local} flags expected, got shape {f.shape}")
        self._ck(self._lib.cellector_set_excluded(self.h, _p(f)))

    def set_loci_mask(self, used):
        """loci_used := used, 1 = used, as loci_mask() returns it (cellector_set_loci_mask)"""
        m = np.ascontiguousarray(np.asarray(used) != 0, dtype=np.uint8)
        if m.shape != (self.dims().loci_used,):
            raise ValueError(f"set_loci_mask: {self.dims().loci_used} entries expected, got shape {m.shape}")
        self._ck(self._lib.cellector_set_loci_mask(self.h, _p(m)))

    def em_reset(self):
        """back to the state the ingest left: empty exclusion set, all loci used, iteration 0 (cellector_em_reset)"""
        self._ck(self._lib.cellector_em_reset(self.h))

    def resolution(self):
        """What option resolve_ties did in the last iteration (cellector_iter_resolution): cells evaluated with the reference's
        arithmetic, exclusion flags it changed, bits 1/2/4 = median/iqr/threshold changed, the option's value."""
        r = Resolution()
        self._ck(self._lib.cellector_iter_resolution(self.h, C.byref(r)))
        return r

    def resolved_cells(self):
        """The local indices of the cells option resolve_ties evaluated in the last iteration (sorted)."""
        ids = np.zeros(self.resolution().n_evaluated, np.uint32)
        if ids.size:
            self._ck(self._lib.cellector_iter_resolved_cells(self.h, _p(ids)))
        return np.sort(ids)

    def cell_outputs(self):
        n = self.n_local
        ll, ell, nl, norm = (np.empty(n, np.float64) for _ in range(4))
        self._ck(self._lib.cellector_iter_cell_outputs(self.h, _p(ll), _p(ell), _p(nl), _p(norm)))
        return dict(ll=ll, expected_ll=ell, loci_used=nl, normalized=norm)

    def locus_outputs(self):
        L = self.dims().loci_used
        cm, cj = np.empty(L, np.float64), np.empty(L, np.float64)
        ints = [np.empty(L, np.uint64) for _ in range(6)]
        self._ck(self._lib.cellector_iter_locus_outputs(self.h, _p(cm), _p(cj), *[_p(a) for a in ints]))
        keys = ["cells_min", "cells_maj", "alt_min", "ref_min", "alt_maj", "ref_maj"]
        return dict(contrib_min=cm, contrib_maj=cj, **dict(zip(keys, ints)))

    def loci_mask(self):
        out = np.empty(self.dims().loci_used, np.uint8)
        self._ck(self._lib.cellector_loci_mask(self.h, _p(out)))
        return out

    def excluded(self):
        out = np.empty(self.n_local, np.uint8)
        self._ck(self._lib.cellector_excluded(self.h, _p(out)))
        return out

    def alpha_betas(self):
        L = self.dims().loci_used
        a, b = np.empty(L, np.float64), np.empty(L, np.float64)
        self._ck(self._lib.cellector_alpha_betas(self.h, _p(a), _p(b)))
        return a, b

    def cell_log_likelihoods(self, alpha, beta, mask=None):
        n = self.n_local
        alpha = np.ascontiguousarray(alpha, np.float64)
        beta = np.ascontiguousarray(beta, np.float64)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        ll, ell, nl = (np.empty(n, np.float64) for _ in range(3))
        self._ck(self._lib.cellector_cell_log_likelihoods(self.h, _p(alpha), _p(beta), _p(mask), _p(ll), _p(ell), _p(nl)))
        return ll, ell, nl

    def cell_pmfs(self, cells, alpha=None, beta=None, mask=None):
        """The reference's PMFData of the listed cells (cellector_cell_pmfs): one record per entry at a used locus, cells in
        list order, entries in the by-cell CSR's order.  alpha / beta / mask default to alpha_betas() and loci_mask(), i.e. the
        records the next em_begin would produce.  Returns a dict of arrays: rec_ptr [len(cells) + 1], then locus_index, alt,
        ref, log_pmf, expected_log_pmf, expected_log_variance of rec_ptr[-1] records each."""
        cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1)
        if alpha is None or beta is None:
            a0, b0 = self.alpha_betas()
            alpha = a0 if alpha is None else alpha
            beta = b0 if beta is None else beta
            mask = self.loci_mask() if mask is None else mask
        alpha = np.ascontiguousarray(alpha, np.float64)
        beta = np.ascontiguousarray(beta, np.float64)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        rp = np.zeros(len(cells) + 1, np.uint64)
        head = (self.h, _p(alpha), _p(beta), _p(mask), _p(cells), len(cells), _p(rp))
        self._ck(self._lib.cellector_cell_pmfs(*head, 0, None, None, None, None, None, None))
        n = int(rp[-1])
        ints = [np.zeros(n, np.uint32) for _ in range(3)]
        flts = [np.zeros(n, np.float64) for _ in range(3)]
        if n:
            self._ck(self._lib.cellector_cell_pmfs(*head, n, *[_p(a) for a in ints + flts]))
        keys = ["locus_index", "alt", "ref", "log_pmf", "expected_log_pmf", "expected_log_variance"]
        return dict(rec_ptr=rp, **dict(zip(keys, ints + flts)))

    def _per_cell_f64(self):
        """an output array of the local cells; None before a load (the library then refuses the call with its own message)"""
        return np.zeros(self.n_local, np.float64) if self.dims().total_cells else None

    def cell_log_variances(self, alpha, beta, mask=None):
        """expected_log_variances, the fourth vector of get_cell_log_likelihoods (main.rs:587), under the given alpha / beta /
        mask (cellector_cell_log_variances): per local cell the sum of cell_pmfs()'s expected_log_variance column.  The ctx is
        left as it was."""
        alpha = np.ascontiguousarray(alpha, np.float64)
        beta = np.ascontiguousarray(beta, np.float64)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        out = self._per_cell_f64()
        self._ck(self._lib.cellector_cell_log_variances(self.h, _p(alpha), _p(beta), _p(mask), _p(out)))
        return out

    def cell_variances(self):
        """The last iteration's expected_log_variances (cellector_iter_cell_variances); an error unless that iteration ran with
        option cell_variance or normalization set."""
        out = self._per_cell_f64()
        self._ck(self._lib.cellector_iter_cell_variances(self.h, _p(out)))
        return out

    _LM_KEYS = ("exp_min", "exp_maj", "var_min", "var_maj")

    def locus_moments(self, alpha, beta, mask, flags):
        """Per used locus the expected log-likelihood contribution and its variance of the flagged cells (min) and of the rest
        (maj) under the given alpha / beta / mask (cellector_locus_moments): what main.rs:398/404 would hold had main.rs:394
        pushed expected_log_pmf, and the matching sums of expected_log_variance.  mask None = all loci used.  Returns a dict of
        four [L] arrays: exp_min, exp_maj, var_min, var_maj.  The ctx is left as it was."""
        L = self.dims().loci_used
        alpha = np.ascontiguousarray(alpha, np.float64)
        beta = np.ascontiguousarray(beta, np.float64)
        mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        flags = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8)
        if alpha.shape != (L,) or beta.shape != (L,) or (mask is not None and mask.shape != (L,)):
            raise ValueError(f"locus_moments: alpha, beta and mask of {L} loci expected")
        if flags.shape != (self.n_local,):
            raise ValueError(f"locus_moments: {self.n_local} flags expected, got shape {flags.shape}")
        out = [np.zeros(L, np.float64) for _ in range(4)]
        self._ck(self._lib.cellector_locus_moments(self.h, _p(alpha), _p(beta), _p(mask), _p(flags), *[_p(a) for a in out]))
        return dict(zip(self._LM_KEYS, out))

    def iter_locus_moments(self):
        """The four vectors of the last finished iteration (cellector_iter_locus_moments): under that iteration's alpha / beta
        and mask and its new exclusion set; an error unless it ran with option locus_moments set."""
        out = [np.zeros(self.dims().loci_used, np.float64) for _ in range(4)]
        self._ck(self._lib.cellector_iter_locus_moments(self.h, *[_p(a) for a in out]))
        return dict(zip(self._LM_KEYS, out))

    def locus_total_counts(self, flags=None):
        """[L, 19] uint32 (cellector_locus_total_counts): entries of the flagged cells (None: all cells) per used locus and
        total alt + ref = 0..17; column 18 = their entries with a larger total."""
        if flags is not None:
            flags = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8)
            if flags.shape != (self.n_local,):
                raise ValueError(f"locus_total_counts: {self.n_local} flags expected, got shape {flags.shape}")
        out = np.zeros((self.dims().loci_used, 19), np.uint32)
        self._ck(self._lib.cellector_locus_total_counts(self.h, _p(flags), _p(out)))
        return out

    @staticmethod
    def locus_zscore(contrib, exp, var, cells):
        """(contrib - exp) / sqrt(var) where cells > 0 and var > 0, else 0: the form of main.rs:317-322 on the locus side"""
        contrib, exp, var = (np.asarray(a, np.float64) for a in (contrib, exp, var))
        ok = (np.asarray(cells) > 0) & (var > 0)
        return np.where(ok, (contrib - exp) / np.sqrt(np.where(ok, var, 1.0)), 0.0)

    def posterior_alpha_betas(self, which):
        """(alpha, beta) of calculate_posteriors' distribution `which` for the current exclusion set: 0 minority, 1 majority,
        2 doublet (cellector_posterior_alpha_betas)"""
        L = self.dims().loci_used
        a, b = np.empty(L, np.float64), np.empty(L, np.float64)
        self._ck(self._lib.cellector_posterior_alpha_betas(self.h, int(which), _p(a), _p(b)))
        return a, b

    def posteriors(self, fetch=True):
        if not fetch:  # (the phase on the device only: benchmarks)
            self._ck(self._lib.cellector_posteriors(self.h, None, None, None, None))
            return None
        n = self.n_local
        p, dp, lmaj, lmin = (np.empty(n, np.float64) for _ in range(4))
        self._ck(self._lib.cellector_posteriors(self.h, _p(p), _p(dp), _p(lmaj), _p(lmin)))
        return dict(posterior=p, doublet_posterior=dp, ll_majority=lmaj, ll_minority=lmin)

    # ---- K-genotype classes: labels 0..K-1 or 255 (unlabelled) per cell; classes.py is the numpy twin
    def _class_args(self, labels, n_classes, scale=None, log_prior=None, mask=None):
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if self.dims().total_cells and labels.shape != (self.n_local,):
            raise ValueError(f"{self.n_local} labels expected, got shape {labels.shape}")
        K, L = int(n_classes), self.dims().loci_used
        vec = []
        for name, v in (("scale", scale), ("log_prior", log_prior)):
            v = None if v is None else np.ascontiguousarray(v, np.float64)
            if v is not None and v.shape != (K,):
                raise ValueError(f"{name}: {K} values expected, got shape {v.shape}")
            vec.append(v)
        mask = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask is not None and mask.shape != (L,):
            raise ValueError(f"mask: {L} entries expected, got shape {mask.shape}")
        return labels, max(K, 0), vec[0], vec[1], mask

    def class_tallies(self, labels, n_classes):
        """(cells [K], alt [K, L], ref [K, L]) uint64: the per-class per-locus allele tallies of a labelling
        (cellector_class_tallies); unlabelled cells (255) are in none"""
        labels, K, _, _, _ = self._class_args(labels, n_classes)
        Ka, L = min(K, 16), self.dims().loci_used
        cells, alt, ref = np.zeros(Ka, np.uint64), np.zeros((Ka, L), np.uint64), np.zeros((Ka, L), np.uint64)
        self._ck(self._lib.cellector_class_tallies(self.h, _p(labels), K, _p(cells), _p(alt), _p(ref)))
        return cells, alt, ref

    def class_alpha_betas(self, labels, n_classes, scale=None):
        """(alpha [K, L], beta [K, L]): alt_k * scale_k + 1, ref_k * scale_k + 1 (cellector_class_alpha_betas)"""
        labels, K, scale, _, _ = self._class_args(labels, n_classes, scale)
        Ka, L = min(K, 16), self.dims().loci_used
        a, b = np.zeros((Ka, L), np.float64), np.zeros((Ka, L), np.float64)
        self._ck(self._lib.cellector_class_alpha_betas(self.h, _p(labels), K, _p(scale), _p(a), _p(b)))
        return a, b

    def class_posteriors(self, labels, n_classes, scale=None, log_prior=None, mask=None):
        """Every cell against the K classes of a labelling (cellector_class_posteriors): dict of ll [K, cells], posterior
        [K, cells], best [cells] uint8, qual [cells] uint64.  mask None = all loci used, as in the reference's posterior phase;
        log_prior None = log((n_k + 1) / (labelled cells + live classes)).  A class without a cell is dead: ll -inf, posterior 0."""
        labels, K, scale, log_prior, mask = self._class_args(labels, n_classes, scale, log_prior, mask)
        Ka, n = min(K, 16), (self.n_local if self.dims().total_cells else 0)  # (before a load the library refuses the call itself)
        ll, post = np.zeros((Ka, n), np.float64), np.zeros((Ka, n), np.float64)
        best, qual = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
        self._ck(self._lib.cellector_class_posteriors(self.h, _p(labels), K, _p(scale), _p(log_prior), _p(mask), _p(ll), _p(post),
                                                      _p(best), _p(qual)))
        return dict(ll=ll, posterior=post, best=best, qual=qual)

    def refine_classes(self, labels, n_classes, scale=None, log_prior=None, mask=None, max_iter=100, min_loci=1):
        """Hard EM over class_posteriors (cellector_refine_classes): every labelled cell with at least min_loci entries at used
        loci moves to its best class until nothing moves or max_iter steps have run.  Returns a dict: labels (the result; the
        argument is not changed), summary (RefineSummary) and ll / posterior / qual of the last step."""
        labels, K, scale, log_prior, mask = self._class_args(labels, n_classes, scale, log_prior, mask)
        labels = labels.copy()
        Ka, n = min(K, 16), (self.n_local if self.dims().total_cells else 0)  # (before a load the library refuses the call itself)
        ll, post, qual = np.zeros((Ka, n), np.float64), np.zeros((Ka, n), np.float64), np.zeros(n, np.uint64)
        s = RefineSummary()
        self._ck(self._lib.cellector_refine_classes(self.h, _p(labels), K, _p(scale), _p(log_prior), _p(mask), int(max_iter),
                                                    int(min_loci), C.byref(s), _p(ll), _p(post), _p(qual)))
        return dict(labels=labels, summary=s, ll=ll, posterior=post, qual=qual)

    # ---- ... and the doublet classes of their K (K - 1) / 2 pairs; held [cells]: non-zero = kept out of every tally
    def _doublet_args(self, labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior, mask):
        labels, K, scale, log_prior, mask = self._class_args(labels, n_classes, scale, log_prior, mask)
        held = None if held is None else np.ascontiguousarray(np.asarray(held) != 0, dtype=np.uint8)
        if held is not None and held.shape != labels.shape:
            raise ValueError(f"held: shape {labels.shape} expected, got {held.shape}")
        Ka = min(K, 16)
        P = Ka * (Ka - 1) // 2
        pair_scale = None if pair_scale is None else np.ascontiguousarray(pair_scale, np.float64)
        if pair_scale is not None and pair_scale.shape != (K,):
            raise ValueError(f"pair_scale: {K} values expected, got shape {pair_scale.shape}")
        log_pair_prior = None if log_pair_prior is None else np.ascontiguousarray(log_pair_prior, np.float64)
        if log_pair_prior is not None and log_pair_prior.shape != (P,):
            raise ValueError(f"log_pair_prior: {P} values expected, got shape {log_pair_prior.shape}")
        return labels, held, K, Ka, P, scale, pair_scale, log_prior, log_pair_prior, mask

    def class_pair_alpha_betas(self, labels, n_classes, held=None, pair_scale=None):
        """dict of alpha [P, L], beta [P, L]: the doublet distributions of the P = K (K - 1) / 2 pairs, row p(a, b) = a (2K - a - 1)
        / 2 + (b - a - 1) (cellector_class_pair_alpha_betas); pair_scale None = every class at the weight of the smallest"""
        labels, held, K, Ka, P, _, pair_scale, _, _, _ = self._doublet_args(labels, held, n_classes, None, pair_scale, None, None, None)
        L = self.dims().loci_used
        a, b = np.zeros((P, L), np.float64), np.zeros((P, L), np.float64)
        self._ck(self._lib.cellector_class_pair_alpha_betas(self.h, _p(labels), _p(held), K, _p(pair_scale), _p(a), _p(b)))
        return dict(alpha=a, beta=b)

    def class_doublets(self, labels, n_classes, held=None, scale=None, pair_scale=None, log_prior=None, log_pair_prior=None, mask=None):
        """Every cell against the K classes of a labelling and the P doublet classes of their pairs (cellector_class_doublets):
        dict of ll [K, cells], ll_pair [P, cells], posterior [K, cells], doublet_posterior, best, best_pair [cells, 2] (255, 255
        without a live pair), call (1 = doublet_posterior > 0.5) and qual."""
        labels, held, K, Ka, P, scale, pair_scale, log_prior, log_pair_prior, mask = self._doublet_args(
            labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior, mask)
        n = self.n_local if self.dims().total_cells else 0  # (before a load the library refuses the call itself)
        ll, llp, post = np.zeros((Ka, n), np.float64), np.zeros((P, n), np.float64), np.zeros((Ka, n), np.float64)
        dp, best, bp = np.zeros(n, np.float64), np.zeros(n, np.uint8), np.zeros((n, 2), np.uint8)
        call, qual = np.zeros(n, np.uint8), np.zeros(n, np.uint64)
        self._ck(self._lib.cellector_class_doublets(self.h, _p(labels), _p(held), K, _p(scale), _p(pair_scale), _p(log_prior),
                                                    _p(log_pair_prior), _p(mask), _p(ll), _p(llp), _p(post), _p(dp), _p(best), _p(bp),
                                                    _p(call), _p(qual)))
        return dict(ll=ll, ll_pair=llp, posterior=post, doublet_posterior=dp, best=best, best_pair=bp, call=call, qual=qual)

    def refine_class_doublets(self, labels, n_classes, held=None, scale=None, pair_scale=None, log_prior=None, log_pair_prior=None,
                              mask=None, doublet_threshold=0.5, max_iter=100, min_loci=1):
        """The held-out refine (cellector_refine_class_doublets): every labelled cell with at least min_loci entries at used loci
        moves to its best class and is held out of the tallies while its doublet posterior exceeds doublet_threshold, until
        nothing changes or max_iter steps have run.  Returns a dict: labels and held (the result; the arguments are not changed),
        summary (RefineDoubletsSummary) and ll / ll_pair / posterior / doublet_posterior / best_pair / qual of the last step."""
        labels, held, K, Ka, P, scale, pair_scale, log_prior, log_pair_prior, mask = self._doublet_args(
            labels, held, n_classes, scale, pair_scale, log_prior, log_pair_prior, mask)
        labels = labels.copy()
        held = np.zeros(labels.shape, np.uint8) if held is None else held.copy()
        n = self.n_local if self.dims().total_cells else 0  # (before a load the library refuses the call itself)
        ll, llp, post = np.zeros((Ka, n), np.float64), np.zeros((P, n), np.float64), np.zeros((Ka, n), np.float64)
        dp, bp, qual = np.zeros(n, np.float64), np.zeros((n, 2), np.uint8), np.zeros(n, np.uint64)
        s = RefineDoubletsSummary()
        self._ck(self._lib.cellector_refine_class_doublets(self.h, _p(labels), _p(held), K, _p(scale), _p(pair_scale), _p(log_prior),
                                                           _p(log_pair_prior), _p(mask), float(doublet_threshold), int(max_iter),
                                                           int(min_loci), C.byref(s), _p(ll), _p(llp), _p(post), _p(dp), _p(bp), _p(qual)))
        return dict(labels=labels, held=held, summary=s, ll=ll, ll_pair=llp, posterior=post, doublet_posterior=dp, best_pair=bp, qual=qual)

    # ---- ... and their genotypes over ALL loci of the matrix; genotypes.py is the numpy twin
    def class_genotypes(self, labels, n_classes, ambient=0.03, gt_threshold=0.99, genotypes=True):
        """The K classes' allele tallies over all loci of the matrix, from the staged COO, and the genotype call of
        output_final_vcf per class and locus (cellector_class_genotypes).  Returns a dict: cells [K + 1], alt / ref [K + 1,
        total_loci] uint64 (slot K: the cells labelled 255) and, with genotypes, gt [K, total_loci] uint8 (1 = 1/1, 2 = 0/1, 3 = 0/0,
        0 = ./.: genotypes.GT_STRINGS), gp [K, total_loci] (the largest of the three posteriors) and gp3 [K, total_loci, 3] (hom-alt,
        het, hom-ref).  Cells held out as doublets are passed as 255."""
        labels, K, _, _, _ = self._class_args(labels, n_classes)
        Ka, TL = min(K, 16), self.dims().total_loci
        cells, alt, ref = np.zeros(Ka + 1, np.uint64), np.zeros((Ka + 1, TL), np.uint64), np.zeros((Ka + 1, TL), np.uint64)
        out = dict(cells=cells, alt=alt, ref=ref)
        if genotypes:
            out.update(gt=np.zeros((Ka, TL), np.uint8), gp=np.zeros((Ka, TL), np.float64), gp3=np.zeros((Ka, TL, 3), np.float64))
        self._ck(self._lib.cellector_class_genotypes(self.h, _p(labels), K, float(ambient), float(gt_threshold), _p(cells), _p(alt),
                                                     _p(ref), _p(out.get("gt")), _p(out.get("gp")), _p(out.get("gp3"))))
        return out

    # ---- genotype clusters without labels: a binomial mixture by annealed soft EM over restarts; cluster.py is the numpy twin
    def _cluster_mask(self, mask):
        L = self.dims().loci_used
        mask = None if mask is None else np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
        if mask is not None and mask.shape != (L,):
            raise ValueError(f"mask: {L} entries expected, got shape {mask.shape}")
        return mask

    def cluster_default_params(self):
        p = ClusterParams()
        self._ck(self._lib.cellector_cluster_default_params(C.byref(p)))
        return p

    def cluster(self, n_clusters, n_restarts=None, seed=4, mask=None, **params):
        """K genotype clusters of the loaded matrix without any labels (cellector_cluster): n_restarts random starts side by side
        (None: min(16, 64 // K)), the best returned.  params: theta_floor, anneal_base, tol, anneal_steps, max_iter, min_loci
        (ClusterParams; the library's defaults otherwise).  Returns a dict: labels [cells] uint8 (255: fewer than min_loci
        entries), ll [K, cells], posterior [K, cells], theta [K, L], objective [R] and summary (ClusterSummary)."""
        K = int(n_clusters)
        R = min(16, 64 // max(K, 1)) if n_restarts is None else int(n_restarts)
        p = self.cluster_default_params()
        for k, v in params.items():
            if k not in dict(ClusterParams._fields_):
                raise TypeError(f"cluster: unknown parameter {k!r}")
            setattr(p, k, v)
        mask = self._cluster_mask(mask)
        Ka, Ra = min(max(K, 0), 16), min(max(R, 0), 64)
        n, L = (self.n_local if self.dims().total_cells else 0), self.dims().loci_used  # (before a load the library refuses the call)
        labels, ll, post = np.zeros(n, np.uint8), np.zeros((Ka, n), np.float64), np.zeros((Ka, n), np.float64)
        theta, obj, s = np.zeros((Ka, L), np.float64), np.zeros(Ra, np.float64), ClusterSummary()
        self._ck(self._lib.cellector_cluster(self.h, max(K, 0), max(R, 0), int(seed), C.byref(p), _p(mask), _p(labels), _p(ll), _p(post),
                                             _p(theta), _p(obj), C.byref(s)))
        return dict(labels=labels, ll=ll, posterior=post, theta=theta, objective=obj, summary=s)

    def cluster_m_step(self, w, mask=None, theta_floor=0.01):
        """One M step from weights w [cells, J] and the tables of its theta (cellector_cluster_m_step): dict of A, T, theta [J, L]
        and tab [L, J, 2] = (log theta, log(1 - theta))."""
        w = np.ascontiguousarray(w, np.float64)
        n, L = (self.n_local if self.dims().total_cells else 0), self.dims().loci_used
        if w.ndim != 2 or (self.dims().total_cells and w.shape[0] != n):
            raise ValueError(f"w: shape ({n}, J) expected, got {w.shape}")
        J = w.shape[1]
        Ja = min(J, 64)
        mask = self._cluster_mask(mask)
        A, T, theta = (np.zeros((Ja, L), np.float64) for _ in range(3))
        tab = np.zeros((L, Ja, 2), np.float64)
        self._ck(self._lib.cellector_cluster_m_step(self.h, _p(w), J, _p(mask), float(theta_floor), _p(A), _p(T), _p(theta), _p(tab)))
        return dict(A=A, T=T, theta=theta, tab=tab)

    def cluster_e_step(self, tab, n_clusters, n_restarts=1, temp=None, mask=None):
        """One E step on the caller's tables tab [L, J, 2], J = K R (cellector_cluster_e_step): dict of s, w [cells, J] and
        objective [R]; temp [cells] >= 1 or None = 1 for every cell."""
        K, R = int(n_clusters), int(n_restarts)
        tab = np.ascontiguousarray(tab, np.float64)
        n, L = (self.n_local if self.dims().total_cells else 0), self.dims().loci_used
        J = K * R
        if 0 < J <= 64 and self.dims().total_cells and tab.shape != (L, J, 2):
            raise ValueError(f"tab: shape ({L}, {J}, 2) expected, got {tab.shape}")
        temp = None if temp is None else np.ascontiguousarray(temp, np.float64)
        if temp is not None and temp.shape != (n,):
            raise ValueError(f"temp: {n} values expected, got shape {temp.shape}")
        mask = self._cluster_mask(mask)
        Ja = min(max(J, 0), 64)
        s, w, obj = np.zeros((n, Ja), np.float64), np.zeros((n, Ja), np.float64), np.zeros(min(max(R, 0), 64), np.float64)
        self._ck(self._lib.cellector_cluster_e_step(self.h, _p(tab), max(K, 0), max(R, 0), _p(temp), _p(mask), _p(s), _p(w), _p(obj)))
        return dict(s=s, w=w, objective=obj)

    # ---- donor demultiplexing: cells and classes against known genotypes gt [D, total_loci] (0 = 0/0, 1 = 0/1, 2 = 1/1, 3 = no
    # call); donors.py is the numpy twin
    def donor_default_params(self):
        p = DonorParams()
        self._ck(self._lib.cellector_donor_default_params(C.byref(p)))
        return p

    def _donor_args(self, gt, mask, params):
        gt = np.ascontiguousarray(gt, dtype=np.uint8)
        TL = self.dims().total_loci
        if gt.ndim != 2 or (self.dims().total_cells and gt.shape[1] != TL):
            raise ValueError(f"gt: shape (D, {TL}) expected, got {gt.shape}")
        p = self.donor_default_params()
        for k, v in params.items():
            if k not in dict(DonorParams._fields_):
                raise TypeError(f"donors: unknown parameter {k!r}")
            setattr(p, k, v)
        return gt, gt.shape[0], self._cluster_mask(mask), p

    def donor_tables(self, gt, mask=None, **params):
        """The packed genotypes and the per-locus tables of the donor calls alone (cellector_donor_tables): dict of tab1 [L, 4, 2],
        tab2 [L, 16, 2] = (log theta, log(1 - theta)) and packed [L, W] uint64, W = ceil(D / 32).  params: err, ambient (DonorParams)."""
        gt, D, mask, p = self._donor_args(gt, mask, params)
        L, W = self.dims().loci_used, (min(max(D, 1), 64) + 31) // 32
        tab1, tab2, packed = np.zeros((L, 4, 2), np.float64), np.zeros((L, 16, 2), np.float64), np.zeros((L, W), np.uint64)
        self._ck(self._lib.cellector_donor_tables(self.h, _p(gt), D, C.byref(p), _p(mask), _p(tab1), _p(tab2), _p(packed)))
        return dict(tab1=tab1, tab2=tab2, packed=packed)

    def _donor_gp_args(self, gp, mask, params):
        gp = np.ascontiguousarray(gp, dtype=np.float32)
        TL = self.dims().total_loci
        if gp.ndim != 3 or gp.shape[2] != 3 or (self.dims().total_cells and gp.shape[1] != TL):
            raise ValueError(f"gp: shape (D, {TL}, 3) expected, got {gp.shape}")
        _, _, mask, p = self._donor_args(np.zeros((1, TL), np.uint8), mask, params)
        return gp, gp.shape[0], mask, p

    def donor_posteriors(self, gt, log_prior=None, anchor=None, mask=None, tables=False, **params):
        """Every cell against D genotyped donors and the D - 1 doublets of its anchor donor with every other one
        (cellector_donor_posteriors).  anchor None = the best singlet.  params: err, ambient, doublet_rate, posterior_threshold,
        min_loci (DonorParams).  Returns a dict: ll, pair_ll, posterior, pair_posterior [cells, D], doublet_posterior, best, second,
        best_pair, n_entries, status (0 singlet, 1 doublet, 2 ambiguous, 255 unassigned), anchor [cells], summary (DonorSummary) and,
        with tables, tab1 / tab2."""
        gt, D, mask, p = self._donor_args(gt, mask, params)
        return self._donor_posteriors(self._lib.cellector_donor_posteriors, gt, D, mask, p, log_prior, anchor, tables)

    def donor_posteriors_gp(self, gp, log_prior=None, anchor=None, mask=None, tables=False, **params):
        """donor_posteriors from genotype probabilities gp [D, total_loci, 3] float32 (cellector_donor_posteriors_gp): a row of
        three NaN is a no-call, any other row three weights >= 0 that need not sum to 1.  The same dict."""
        gp, D, mask, p = self._donor_gp_args(gp, mask, params)
        return self._donor_posteriors(self._lib.cellector_donor_posteriors_gp, gp, D, mask, p, log_prior, anchor, tables)

    def donor_weights(self, gp):
        """(w [L, D, 3] float64, kind [L, D] uint8) over the used loci as the device holds them (cellector_donor_weights): kind 0, 1,
        2 = a one-hot row of that genotype, 3 = a no-call (w 0), 4 = a soft row."""
        gp, D, _, _ = self._donor_gp_args(gp, None, {})
        L, Da = self.dims().loci_used, min(max(D, 1), 64)
        w, kind = np.zeros((L, Da, 3), np.float64), np.zeros((L, Da), np.uint8)
        self._ck(self._lib.cellector_donor_weights(self.h, _p(gp), D, _p(w), _p(kind)))
        return w, kind

    def _donor_posteriors(self, call, gt, D, mask, p, log_prior, anchor, tables):
        Da = min(max(D, 1), 64)
        n, L = (self.n_local if self.dims().total_cells else 0), self.dims().loci_used  # (before a load the library refuses the call)
        log_prior = None if log_prior is None else np.ascontiguousarray(log_prior, np.float64)
        if log_prior is not None and log_prior.shape != (D,):
            raise ValueError(f"log_prior: {D} values expected, got shape {log_prior.shape}")
        anchor = None if anchor is None else np.ascontiguousarray(anchor, np.uint8)
        if anchor is not None and anchor.shape != (n,):
            raise ValueError(f"anchor: {n} values expected, got shape {anchor.shape}")
        out = {k: np.zeros((n, Da), np.float64) for k in ("ll", "pair_ll", "posterior", "pair_posterior")}
        out["doublet_posterior"] = np.zeros(n, np.float64)
        for k in ("best", "second", "best_pair"):
            out[k] = np.zeros(n, np.uint8)
        out["n_entries"] = np.zeros(n, np.uint32)
        out["status"], out["anchor"] = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        if tables:
            out["tab1"], out["tab2"] = np.zeros((L, 4, 2), np.float64), np.zeros((L, 16, 2), np.float64)
        s = DonorSummary()
        self._ck(call(
            self.h, _p(gt), D, C.byref(p), _p(log_prior), _p(anchor), _p(mask), _p(out["ll"]), _p(out["pair_ll"]), _p(out["posterior"]),
            _p(out["pair_posterior"]), _p(out["doublet_posterior"]), _p(out["best"]), _p(out["second"]), _p(out["best_pair"]),
            _p(out["n_entries"]), _p(out["status"]), _p(out["anchor"]), C.byref(s), _p(out.get("tab1")), _p(out.get("tab2"))))
        out["summary"] = s
        return out

    # ---- donor panels: up to 4096 donors, pairs of the anchor with a shortlist; donors.py (panel_posteriors) is the twin
    def donor_panel(self, gt, shortlist=8, log_prior=None, anchor=None, mask=None, ll=False, tables=False, **params):
        """Every cell against a panel of D <= 4096 genotyped donors and the doublets of its anchor donor with the M = min(shortlist, D)
        best singlets of the cell (cellector_donor_panel).  Returns a dict: cand [cells, M] uint16 (the shortlist in ascending donor
        index), cand_ll, cand_pair_ll, cand_posterior, cand_pair_posterior [cells, M], doublet_posterior, best_posterior, best, second,
        best_pair (uint16, 65535 = none), anchor, n_entries, status [cells], donor_cells [D] (status-0 cells per best donor), summary
        (DonorPanelSummary) and, with ll, ll [cells, D]; with tables, packed [L, W], tab1 and tab2."""
        gt, D, mask, p = self._donor_args(gt, mask, params)
        shortlist = int(shortlist)
        Da, M = min(max(D, 1), 4096), min(max(shortlist, 1), 64, max(D, 1))
        n, L = (self.n_local if self.dims().total_cells else 0), self.dims().loci_used
        log_prior = None if log_prior is None else np.ascontiguousarray(log_prior, np.float64)
        if log_prior is not None and log_prior.shape != (D,):
            raise ValueError(f"log_prior: {D} values expected, got shape {log_prior.shape}")
        anchor = None if anchor is None else np.ascontiguousarray(anchor, np.uint16)
        if anchor is not None and anchor.shape != (n,):
            raise ValueError(f"anchor: {n} values expected, got shape {anchor.shape}")
        out = dict(cand=np.zeros((n, M), np.uint16))
        for k in ("cand_ll", "cand_pair_ll", "cand_posterior", "cand_pair_posterior"):
            out[k] = np.zeros((n, M), np.float64)
        out["doublet_posterior"], out["best_posterior"] = np.zeros(n, np.float64), np.zeros(n, np.float64)
        for k in ("best", "second", "best_pair", "anchor"):
            out[k] = np.zeros(n, np.uint16)
        out["n_entries"], out["status"] = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        out["donor_cells"] = np.zeros(Da, np.uint64)
        if ll:
            out["ll"] = np.zeros((n, Da), np.float64)
        if tables:
            out["packed"] = np.zeros((L, (Da + 31) // 32), np.uint64)
            out["tab1"], out["tab2"] = np.zeros((L, 4, 2), np.float64), np.zeros((L, 16, 2), np.float64)
        s = DonorPanelSummary()
        self._ck(self._lib.cellector_donor_panel(
            self.h, _p(gt), D, max(shortlist, 0), C.byref(p), _p(log_prior), _p(anchor), _p(mask), _p(out["cand"]), _p(out["cand_ll"]),
            _p(out["cand_pair_ll"]), _p(out["cand_posterior"]), _p(out["cand_pair_posterior"]), _p(out["doublet_posterior"]),
            _p(out["best_posterior"]), _p(out["best"]), _p(out["second"]), _p(out["best_pair"]), _p(out["anchor"]), _p(out["n_entries"]),
            _p(out["status"]), _p(out["donor_cells"]), C.byref(s), _p(out.get("ll")), _p(out.get("packed")), _p(out.get("tab1")),
            _p(out.get("tab2"))))
        out["summary"] = s
        return out

    def match_donors_panel(self, labels, n_classes, gt, mask=None, **params):
        """match_donors for a panel of D <= 4096 donors (cellector_match_donors_panel): the same dict, best uint16 (65535: a class
        without a cell)"""
        labels, K, _, _, _ = self._class_args(labels, n_classes)
        gt, D, mask, p = self._donor_args(gt, mask, params)
        Ka, Da = min(K, 16), min(max(D, 1), 4096)
        ll, best, margin, cells = np.zeros((Ka, Da), np.float64), np.zeros(Ka, np.uint16), np.zeros(Ka, np.float64), np.zeros(Ka, np.uint64)
        self._ck(self._lib.cellector_match_donors_panel(self.h, _p(labels), K, _p(gt), D, C.byref(p), _p(mask), _p(ll), _p(best), _p(margin),
                                                        _p(cells)))
        return dict(ll=ll, best=best, margin=margin, cells=cells)

    # ---- the fit of the called hypothesis: cells no genotyped donor explains; donors.py (moment_tables, fit_sums, fit) is the twin
    def donor_fit_default_params(self):
        p = DonorFitParams()
        self._ck(self._lib.cellector_donor_fit_default_params(C.byref(p)))
        return p

    def donor_moment_tables(self, mask=None, **params):
        """The moment tables of the donor fit alone (cellector_donor_moment_tables): (mom1 [L, 4, 2], mom2 [L, 16, 2]) = (h, v), the
        mean and the variance of an entry's term per read under the row's theta.  params: err, ambient (DonorParams)."""
        TL = self.dims().total_loci
        _, _, mask, p = self._donor_args(np.zeros((1, TL), np.uint8), mask, params)
        L = self.dims().loci_used
        mom1, mom2 = np.zeros((L, 4, 2), np.float64), np.zeros((L, 16, 2), np.float64)
        self._ck(self._lib.cellector_donor_moment_tables(self.h, C.byref(p), _p(mask), _p(mom1), _p(mom2)))
        return mom1, mom2

    def donor_fit(self, gt, log_prior=None, anchor=None, mask=None, tables=False, **params):
        """How well the hypothesis the donor call chose explains every cell (cellector_donor_fit): z = (ll - expected) /
        sqrt(variance) under it, and the cells whose z lies below q1 - iqr_multiple iqr of the singlets' flagged unmatched: cells of
        a donor gt does not hold.  params: DonorParams' and iqr_multiple, min_cells (DonorFitParams).  Returns a dict: fit_e, fit_v,
        pair_e, pair_v, z, pair_z [cells, D], call_z, hyp_a, hyp_b (255: a singlet hypothesis), status, unmatched [cells], summary
        (DonorFitSummary) and, with tables, mom1 / mom2."""
        fit = self.donor_fit_default_params()
        for k in [k for k in params if k in dict(DonorFitParams._fields_)]:
            setattr(fit, k, params.pop(k))
        gt, D, mask, p = self._donor_args(gt, mask, params)
        Da = min(max(D, 1), 64)
        n, L = (self.n_local if self.dims().total_cells else 0), self.dims().loci_used
        log_prior = None if log_prior is None else np.ascontiguousarray(log_prior, np.float64)
        if log_prior is not None and log_prior.shape != (D,):
            raise ValueError(f"log_prior: {D} values expected, got shape {log_prior.shape}")
        anchor = None if anchor is None else np.ascontiguousarray(anchor, np.uint8)
        if anchor is not None and anchor.shape != (n,):
            raise ValueError(f"anchor: {n} values expected, got shape {anchor.shape}")
        out = {k: np.zeros((n, Da), np.float64) for k in ("fit_e", "fit_v", "pair_e", "pair_v", "z", "pair_z")}
        out["call_z"] = np.zeros(n, np.float64)
        for k in ("hyp_a", "hyp_b", "status", "unmatched"):
            out[k] = np.zeros(n, np.uint8)
        if tables:
            out["mom1"], out["mom2"] = np.zeros((L, 4, 2), np.float64), np.zeros((L, 16, 2), np.float64)
        s = DonorFitSummary()
        self._ck(self._lib.cellector_donor_fit(
            self.h, _p(gt), D, C.byref(p), C.byref(fit), _p(log_prior), _p(anchor), _p(mask), _p(out["fit_e"]), _p(out["fit_v"]),
            _p(out["pair_e"]), _p(out["pair_v"]), _p(out["z"]), _p(out["pair_z"]), _p(out["call_z"]), _p(out["hyp_a"]), _p(out["hyp_b"]),
            _p(out["status"]), _p(out["unmatched"]), C.byref(s), _p(out.get("mom1")), _p(out.get("mom2"))))
        out["summary"] = s
        return out

    def match_donors(self, labels, n_classes, gt, mask=None, **params):
        """The K classes of a labelling against D genotyped donors (cellector_match_donors): dict of ll [K, D], best [K] uint8 (255:
        a class without a cell), margin [K] (best minus runner-up) and cells [K].  Two classes may name the same donor."""
        labels, K, _, _, _ = self._class_args(labels, n_classes)
        gt, D, mask, p = self._donor_args(gt, mask, params)
        Ka, Da = min(K, 16), min(max(D, 1), 64)
        ll, best, margin, cells = np.zeros((Ka, Da), np.float64), np.zeros(Ka, np.uint8), np.zeros(Ka, np.float64), np.zeros(Ka, np.uint64)
        self._ck(self._lib.cellector_match_donors(self.h, _p(labels), K, _p(gt), D, C.byref(p), _p(mask), _p(ll), _p(best), _p(margin),
                                                  _p(cells)))
        return dict(ll=ll, best=best, margin=margin, cells=cells)

    def match_donors_gp(self, labels, n_classes, gp, mask=None, **params):
        """match_donors from genotype probabilities gp [D, total_loci, 3] (cellector_match_donors_gp): the same dict"""
        labels, K, _, _, _ = self._class_args(labels, n_classes)
        gp, D, mask, p = self._donor_gp_args(gp, mask, params)
        Ka, Da = min(K, 16), min(max(D, 1), 64)
        ll, best, margin, cells = np.zeros((Ka, Da), np.float64), np.zeros(Ka, np.uint8), np.zeros(Ka, np.float64), np.zeros(Ka, np.uint64)
        self._ck(self._lib.cellector_match_donors_gp(self.h, _p(labels), K, _p(gp), D, C.byref(p), _p(mask), _p(ll), _p(best), _p(margin),
                                                     _p(cells)))
        return dict(ll=ll, best=best, margin=margin, cells=cells)

    # ---- ambient fraction estimation: the cells of every source scored at G ambient fractions at once; gt [S, total_loci] coded as
    # for the donor calls, assign [cells] uint8 (255: the cell takes no part); ambient.py is the numpy twin
    def ambient_default_params(self):
        p = AmbientParams()
        self._ck(self._lib.cellector_ambient_default_params(C.byref(p)))
        return p

    def _ambient_args(self, gt, assign, mask):
        gt = np.ascontiguousarray(gt, dtype=np.uint8)
        TL = self.dims().total_loci
        n = self.n_local if self.dims().total_cells else 0  # (before a load the library refuses the call)
        if gt.ndim != 2 or (self.dims().total_cells and gt.shape[1] != TL):
            raise ValueError(f"gt: shape (S, {TL}) expected, got {gt.shape}")
        assign = np.ascontiguousarray(assign, dtype=np.uint8)
        if self.dims().total_cells and assign.shape != (n,):
            raise ValueError(f"assign: {n} values expected, got shape {assign.shape}")
        return gt, gt.shape[0], assign, self._cluster_mask(mask), n

    def ambient_tables(self, rho, err=0.01, mask=None):
        """The per-locus tables of one grid of ambient fractions alone (cellector_ambient_tables): dict of tab [L, 4, G, 2] = (log theta,
        log(1 - theta)), theta = (1 - rho_j) e_g + rho_j soup."""
        rho = np.ascontiguousarray(rho, np.float64)
        if rho.ndim != 1:
            raise ValueError(f"rho: one dimension expected, got shape {rho.shape}")
        G = len(rho)
        tab = np.zeros((self.dims().loci_used, 4, min(max(G, 1), 32), 2), np.float64)
        self._ck(self._lib.cellector_ambient_tables(self.h, _p(rho), G, float(err), _p(self._cluster_mask(mask)), _p(tab)))
        return dict(tab=tab)

    def ambient_profile(self, gt, assign, rho, err=0.01, min_loci=1, mask=None, tables=False):
        """The profile log-likelihood over a caller's grid rho [G] (cellector_ambient_profile).  Returns a dict: ll [cells, G], total
        [G], source_total [S, G], source_cells [S], n_entries, cell_rho, cell_se [cells] (NaN for a cell that takes no part or has
        fewer than min_loci entries) and, with tables, tab [L, 4, G, 2]."""
        gt, S, assign, mask, n = self._ambient_args(gt, assign, mask)
        rho = np.ascontiguousarray(rho, np.float64)
        if rho.ndim != 1:
            raise ValueError(f"rho: one dimension expected, got shape {rho.shape}")
        G = len(rho)
        Ga, Sa = min(max(G, 1), 32), min(max(S, 1), 64)
        out = dict(ll=np.zeros((n, Ga), np.float64), total=np.zeros(Ga, np.float64), source_total=np.zeros((Sa, Ga), np.float64),
                   source_cells=np.zeros(Sa, np.uint64), n_entries=np.zeros(n, np.uint32), cell_rho=np.zeros(n, np.float64),
                   cell_se=np.zeros(n, np.float64))
        if tables:
            out["tab"] = np.zeros((self.dims().loci_used, 4, Ga, 2), np.float64)
        self._ck(self._lib.cellector_ambient_profile(
            self.h, _p(gt), S, _p(assign), _p(rho), G, float(err), int(min_loci), _p(mask), _p(out["ll"]), _p(out["total"]),
            _p(out["source_total"]), _p(out["source_cells"]), _p(out["n_entries"]), _p(out["cell_rho"]), _p(out["cell_se"]),
            _p(out.get("tab"))))
        return out

    def estimate_ambient(self, gt, assign, mask=None, **params):
        """The pool's ambient fraction by a grid search that zooms in (cellector_estimate_ambient).  params: err, lo, hi, grid, rounds,
        min_loci (AmbientParams).  Returns a dict: rho, se, curvature, log_likelihood, lo, hi, j_star, at_boundary, rounds,
        n_cells_used, source_rho, source_se, source_cells [S], the first round's cell_rho, cell_se, n_entries [cells], and summary
        (AmbientSummary)."""
        gt, S, assign, mask, n = self._ambient_args(gt, assign, mask)
        p = self.ambient_default_params()
        for k, v in params.items():
            if k not in dict(AmbientParams._fields_):
                raise TypeError(f"ambient: unknown parameter {k!r}")
            setattr(p, k, v)
        s = AmbientSummary()
        cell_rho, cell_se, cnt = np.zeros(n, np.float64), np.zeros(n, np.float64), np.zeros(n, np.uint32)
        self._ck(self._lib.cellector_estimate_ambient(self.h, _p(gt), S, _p(assign), C.byref(p), _p(mask), C.byref(s), _p(cell_rho),
                                                      _p(cell_se), _p(cnt)))
        Sa = min(max(S, 0), 64)
        out = {k: getattr(s, k) for k in ("rho", "se", "curvature", "log_likelihood", "lo", "hi", "j_star", "at_boundary", "rounds",
                                          "n_cells_used")}
        out.update(source_rho=np.array(s.source_rho[:Sa]), source_se=np.array(s.source_se[:Sa]),
                   source_cells=np.array(s.source_cells[:Sa], np.uint64), cell_rho=cell_rho, cell_se=cell_se, n_entries=cnt, summary=s)
        return out

    # ---- donor pair fractions: every cell under a pair of donors (pair_a, pair_b [cells] uint8, pair_a 255: the cell takes no part)
    # at G shares f of donor a at once; pair_fraction.py is the numpy twin
    def pair_fraction_default_params(self):
        p = PairFractionParams()
        self._ck(self._lib.cellector_pair_fraction_default_params(C.byref(p)))
        return p

    @staticmethod
    def _pair_fraction_grid(frac):
        if frac is None:
            return None, 17
        frac = np.ascontiguousarray(frac, np.float64)
        if frac.ndim != 1:
            raise ValueError(f"frac: one dimension expected, got shape {frac.shape}")
        return frac, len(frac)

    def pair_fraction_tables(self, frac=None, mask=None, donor_params=None):
        """The per-locus tables of one grid of pair fractions alone (cellector_pair_fraction_tables): dict of tab [L, 16, G, 2] = (log
        theta, log(1 - theta)) at index 4 g_a + g_b, theta = f_j theta_ga + (1 - f_j) theta_gb, and frac [G], the grid used (None:
        j / 16).  donor_params: a dict of err, ambient (DonorParams)."""
        TL = self.dims().total_loci
        _, _, mask, p = self._donor_args(np.zeros((1, TL), np.uint8), mask, dict(donor_params or {}))
        frac, G = self._pair_fraction_grid(frac)
        tab = np.zeros((self.dims().loci_used, 16, min(max(G, 1), 32), 2), np.float64)
        self._ck(self._lib.cellector_pair_fraction_tables(self.h, C.byref(p), _p(frac), G, _p(mask), _p(tab)))
        return dict(tab=tab, frac=np.arange(17) / 16.0 if frac is None else frac)

    def donor_pair_fractions(self, gt, pair_a, pair_b, frac=None, params=None, donor_params=None, mask=None, tables=False):
        """The share of every cell's reads that come from donor pair_a[c] of its pair (pair_a[c], pair_b[c]), profiled over the grid
        frac [G] (cellector_donor_pair_fractions; None: j / 16, j = 0 ... 16).  params: a dict of min_fraction, min_loci
        (PairFractionParams); donor_params: a dict of err, ambient (DonorParams).  Returns a dict: ll [cells, G], n_entries,
        cell_frac, cell_se (NaN for a cell that takes no part or has fewer than min_loci entries), j_star, kind (0 balanced, 1 toward
        a, 2 toward b, 3 flat, 255 no part) [cells], frac [G], summary (PairFractionSummary) and, with tables, tab [L, 16, G, 2]."""
        gt, D, mask, p = self._donor_args(gt, mask, dict(donor_params or {}))
        fp = self.pair_fraction_default_params()
        for k, v in dict(params or {}).items():
            if k not in dict(PairFractionParams._fields_):
                raise TypeError(f"pair fractions: unknown parameter {k!r}")
            setattr(fp, k, v)
        n = self.n_local if self.dims().total_cells else 0  # (before a load the library refuses the call)
        pair_a, pair_b = np.ascontiguousarray(pair_a, np.uint8), np.ascontiguousarray(pair_b, np.uint8)
        for name, v in (("pair_a", pair_a), ("pair_b", pair_b)):
            if self.dims().total_cells and v.shape != (n,):
                raise ValueError(f"{name}: {n} values expected, got shape {v.shape}")
        frac, G = self._pair_fraction_grid(frac)
        Ga = min(max(G, 1), 32)
        out = dict(ll=np.zeros((n, Ga), np.float64), n_entries=np.zeros(n, np.uint32), cell_frac=np.zeros(n, np.float64),
                   cell_se=np.zeros(n, np.float64), j_star=np.zeros(n, np.uint8), kind=np.zeros(n, np.uint8))
        if tables:
            out["tab"] = np.zeros((self.dims().loci_used, 16, Ga, 2), np.float64)
        s = PairFractionSummary()
        self._ck(self._lib.cellector_donor_pair_fractions(
            self.h, _p(gt), D, C.byref(p), C.byref(fp), _p(pair_a), _p(pair_b), _p(frac), G, _p(mask), _p(out["ll"]), _p(out["n_entries"]),
            _p(out["cell_frac"]), _p(out["cell_se"]), _p(out["j_star"]), _p(out["kind"]), C.byref(s), _p(out.get("tab"))))
        out["frac"] = np.arange(17) / 16.0 if frac is None else frac
        out["summary"] = s
        return out

    # ---- donor genotype refinement: the donors' genotypes from the reads of the cells called for them; donor_genotypes.py is the
    # numpy twin
    def donor_genotypes_default_params(self):
        p = DonorGenotypesParams()
        self._ck(self._lib.cellector_donor_genotypes_default_params(C.byref(p)))
        return p

    def donor_genotypes(self, assign, prior=None, n_donors=None, posterior=True, timing=False, **params):
        """The D donors' genotypes over all loci of the matrix from the reads of the cells assigned to them
        (cellector_donor_genotypes).  assign [cells] uint8: a donor, or 255 = no part; prior [D, total_loci, 3] float32 (three NaN: a
        no-call) or None = no calls at all, then n_donors names D.  params: err, ambient, gt_threshold, prior_floor
        (DonorGenotypesParams).  Returns a dict: cells [D + 1], alt / ref [D + 1, total_loci] uint64 (slot D: the cells assigned 255)
        and, with posterior, q [D, total_loci, 3], gt_out, kind [D, total_loci] uint8 (0 no reads, 1 confirmed, 2 filled, 3 changed,
        4 withdrawn), tab [total_loci, 3, 2] and summary (a dict of [D] arrays); with timing, pass_ms [2]."""
        TL = self.dims().total_loci
        n = self.n_local if self.dims().total_cells else 0  # (before a load the library refuses the call)
        assign = np.ascontiguousarray(assign, np.uint8)
        if self.dims().total_cells and assign.shape != (n,):
            raise ValueError(f"assign: {n} values expected, got shape {assign.shape}")
        if prior is not None:
            prior = np.ascontiguousarray(prior, np.float32)
            if prior.ndim != 3 or prior.shape[2] != 3 or (self.dims().total_cells and prior.shape[1] != TL):
                raise ValueError(f"prior: shape (D, {TL}, 3) expected, got {prior.shape}")
            if n_donors is not None and int(n_donors) != prior.shape[0]:
                raise ValueError(f"n_donors = {n_donors}, but prior holds {prior.shape[0]} donors")
            D = prior.shape[0]
        elif n_donors is None:
            raise ValueError("n_donors: needed when prior is None")
        else:
            D = int(n_donors)
        p = self.donor_genotypes_default_params()
        for k, v in params.items():
            if k not in dict(DonorGenotypesParams._fields_):
                raise TypeError(f"donor genotypes: unknown parameter {k!r}")
            setattr(p, k, v)
        Da = min(max(D, 1), 64)
        out = dict(cells=np.zeros(Da + 1, np.uint64), alt=np.zeros((Da + 1, TL), np.uint64), ref=np.zeros((Da + 1, TL), np.uint64))
        s = DonorGenotypesSummary()
        if posterior:
            out.update(q=np.zeros((Da, TL, 3), np.float64), gt_out=np.zeros((Da, TL), np.uint8), kind=np.zeros((Da, TL), np.uint8),
                       tab=np.zeros((TL, 3, 2), np.float64))
        if timing:
            out["pass_ms"] = np.zeros(2, np.float64)
        self._ck(self._lib.cellector_donor_genotypes(
            self.h, _p(assign), _p(prior), max(D, 0), C.byref(p), _p(out["cells"]), _p(out["alt"]), _p(out["ref"]), _p(out.get("q")),
            _p(out.get("gt_out")), _p(out.get("kind")), C.byref(s) if posterior else None, _p(out.get("tab")), _p(out.get("pass_ms"))))
        if posterior:
            out["summary"] = s.as_dict(Da)
        return out

    def refine_donors(self, prior, max_iter=10, log_prior=None, mask=None, donor_params=None, **params):
        """Calls and genotypes in turn, a plain loop: donor_posteriors_gp under the current rows, donor_genotypes on the status-0 cells
        under their best donor with the CALLER's prior, to_gp(q) as the next round's rows; it stops when no cell's (status, best)
        changes, or after max_iter rounds.  donor_params: a dict for the donor call (DonorParams; err and ambient go to both calls
        unless params names its own).  Returns (the last donor result, the last genotype result, the rounds run)."""
        from . import donor_genotypes as dg
        prior = np.ascontiguousarray(prior, np.float32)
        dp = dict(donor_params or {})
        gparams = {k: dp[k] for k in ("err", "ambient") if k in dp}
        gparams.update(params)
        gp, last, don, gen, rounds = prior, None, None, None, 0
        for rounds in range(1, int(max_iter) + 1):
            don = self.donor_posteriors_gp(gp, log_prior=log_prior, mask=mask, **dp)
            key = (don["status"], don["best"])
            if last is not None and np.array_equal(key[0], last[0]) and np.array_equal(key[1], last[1]):
                break
            last = key
            assign = np.where(don["status"] == 0, don["best"], 255).astype(np.uint8)
            gen = self.donor_genotypes(assign, prior, **gparams)
            gp = dg.to_gp(gen["q"])
        return don, gen, rounds

    def assign(self, posterior_threshold=0.999, min_loci_used=30):
        """calculate_posteriors + the labelling rule of output_final_assignments in one call (cellector_assign).  With option
        resolve_posteriors 1 / 2 the evaluated cells' values, labels and quals are the reference's (assign_resolution())."""
        n = self.n_local
        p, dp, lmaj, lmin = (np.empty(n, np.float64) for _ in range(4))
        pa, aa, q = np.empty(n, np.uint8), np.empty(n, np.uint8), np.empty(n, np.uint64)
        self._ck(self._lib.cellector_assign(self.h, float(posterior_threshold), int(min_loci_used), _p(p), _p(dp), _p(lmaj),
                                            _p(lmin), _p(pa), _p(aa), _p(q)))
        return dict(posterior=p, doublet_posterior=dp, ll_majority=lmaj, ll_minority=lmin, posterior_assignment=pa,
                    anomaly_assignment=aa, qual=q)

    def assign_resolution(self):
        """What option resolve_posteriors did in the last assign(): cells evaluated with the reference's arithmetic, how many
        of their labels / quals differ from the ones the device's own values give, the option's value."""
        r = AssignResolution()
        self._ck(self._lib.cellector_assign_resolution(self.h, C.byref(r)))
        return r

    def assign_resolved_cells(self):
        """The local indices of the cells the last assign() evaluated (sorted)."""
        ids = np.zeros(self.assign_resolution().n_evaluated, np.uint32)
        if ids.size:
            self._ck(self._lib.cellector_assign_resolved_cells(self.h, _p(ids)))
        return np.sort(ids)

    def final_allele_tallies(self):
        tl = self.dims().total_loci
        outs = [np.empty(tl, np.uint64) for _ in range(4)]
        self._ck(self._lib.cellector_final_allele_tallies(self.h, *[_p(o) for o in outs]))
        return dict(zip(["alt_min", "ref_min", "alt_maj", "ref_maj"], outs))

    def engine_info(self):
        e = EngineInfo()
        self._ck(self._lib.cellector_engine_info(self.h, C.byref(e)))
        return e

    def order_statistics(self, keys, iqr_multiple=5.0):
        """(median, iqr, threshold) of the keys by the device select (a multi-device ctx: the sharded select)."""
        keys = np.ascontiguousarray(keys, dtype=np.float64)
        out = np.zeros(3, dtype=np.float64)
        self._ck(self._lib.cellector_order_statistics(self.h, keys.ctypes.data, len(keys), float(iqr_multiple), out.ctypes.data))
        return tuple(out.tolist())

    # ---- timing
    def kernel_time(self, which):
        ms, n = C.c_double(), C.c_uint64()
        self._ck(self._lib.cellector_kernel_time(self.h, which, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def reset_timing(self):
        self._ck(self._lib.cellector_reset_timing(self.h))


def device_count():
    n = C.c_int(0)
    load_library().cellector_device_count(C.byref(n))
    return n.value


def comm_unique_id():
    """128 opaque bytes (ncclUniqueId) for Cellector.comm_init_rank; made on rank 0, broadcast by the host"""
    buf = (C.c_char * 128)()
    st = load_library().cellector_comm_unique_id(buf)
    if st != 0:
        raise CellectorError(st, "cellector_comm_unique_id failed (RCCL not loadable?)")
    return bytes(buf)


def assignments(posterior, doublet_posterior, entries_per_cell, excluded, posterior_threshold=0.999,
                min_loci_used=30):
    """The labelling rule of output_final_assignments (main.rs:141-171) on host arrays.

    Returns (posterior_assignment, anomaly_assignment, qual): codes 0 -> "0" (minority), 1 -> "1" (majority),
    2 -> "doublet", 3 -> "unassigned"; anomaly 0 if the cell is in the final exclusion set else 1.
    """
    p = np.asarray(posterior, np.float64)
    pa = np.full(p.shape, 3, np.uint8)
    pa[(1.0 - p) > posterior_threshold] = 1
    pa[p > posterior_threshold] = 0
    pa[np.asarray(doublet_posterior) > 0.5] = 2
    pa[np.asarray(entries_per_cell) < min_loci_used] = 3
    aa = np.where(np.asarray(excluded) != 0, 0, 1).astype(np.uint8)
    post = np.fmax(p, 1.0 - p)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.fmin(-10.0 * np.log10(1.0 - post), 255.0)
    q = np.where(np.isnan(q) | (q < 0), 0.0, q)
    return pa, aa, q.astype(np.uint64)
