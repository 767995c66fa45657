"""ctypes binding of libipkgpu.so (include/ipkgpu.h).

Mirrors the seam of ipk/src/db_builder.cpp:576-698: ``Engine.score_groups`` takes the ghost-node
matrices of a batch of branch groups and returns, per branch id, the max-reduced (key, score) set
that ``explore_group`` leaves in ``group_map`` (db_builder.cpp:685), plus the number of scored
phylo-k-mers (the reference's ``count``, db_builder.cpp:664).
"""
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "libipkgpu.so")
_lib = None

T_TOTAL, T_PREFIX, T_SCORE, T_COMPACT, T_SCORE_LAUNCHES, T_SCORE_MAIN, T_SCORE_REDUCE, T_XP_COUNT, T_XP_WRITE, T_KM_WRITE = range(10)

# every symbol include/ipkgpu.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "ipkgpu_create", "ipkgpu_destroy", "ipkgpu_last_error", "ipkgpu_last_main_kernel", "ipkgpu_last_tables_compressed", "ipkgpu_set_option",
    "ipkgpu_log_threshold", "ipkgpu_bits_per_symbol", "ipkgpu_kmer_batch", "ipkgpu_max_k",
    "ipkgpu_score_groups", "ipkgpu_score_groups_device",
    "ipkgpu_result_num_groups", "ipkgpu_result_group_ids", "ipkgpu_result_offsets",
    "ipkgpu_result_emitted", "ipkgpu_result_keys", "ipkgpu_result_scores",
    "ipkgpu_result_keys_device", "ipkgpu_result_scores_device", "ipkgpu_result_time_ms",
    "ipkgpu_result_free", "ipkgpu_score_groups_positions", "ipkgpu_result_positions", "ipkgpu_debug_exec_violations",
]


class IpkGpuError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"ipkgpu error {code}: {message}")
        self.code = code


def load_library():
    """Loads libipkgpu.so (fails loudly if the HIP extension has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(f"{_LIB_PATH} is missing: build it with `python -m ipk_amd.build` "
                          "(there is no CPU fallback)")
    # torch ships its own HIP runtime under the same SONAME; import it first so that one copy
    # of libamdhip64 serves both torch tensors and this library.
    try:
        import torch  # noqa: F401
    except Exception:  # pragma: no cover - torch is optional for the C ABI itself
        pass
    # IPKGPU_LIB: an alternative build of the same library (tuning experiments only)
    L = C.CDLL(os.environ.get("IPKGPU_LIB") or _LIB_PATH)
    f32p, u32p, u64p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.ipkgpu_create.restype = C.c_int
    L.ipkgpu_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.ipkgpu_destroy.restype = None
    L.ipkgpu_destroy.argtypes = [C.c_void_p]
    L.ipkgpu_last_error.restype = C.c_char_p
    L.ipkgpu_last_error.argtypes = [C.c_void_p]
    L.ipkgpu_last_main_kernel.restype = C.c_char_p
    L.ipkgpu_last_main_kernel.argtypes = [C.c_void_p]
    L.ipkgpu_last_tables_compressed.restype = C.c_int
    L.ipkgpu_last_tables_compressed.argtypes = [C.c_void_p]
    L.ipkgpu_debug_exec_violations.restype = C.c_int64
    L.ipkgpu_debug_exec_violations.argtypes = [C.c_void_p]
    L.ipkgpu_set_option.restype = C.c_int
    L.ipkgpu_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    L.ipkgpu_log_threshold.restype = C.c_float
    L.ipkgpu_log_threshold.argtypes = [C.c_float, C.c_uint32, C.c_uint32]
    L.ipkgpu_bits_per_symbol.restype = C.c_uint32
    L.ipkgpu_bits_per_symbol.argtypes = [C.c_uint32]
    L.ipkgpu_kmer_batch.restype = C.c_size_t
    L.ipkgpu_kmer_batch.argtypes = [C.c_uint32, C.c_size_t]
    L.ipkgpu_max_k.restype = C.c_uint32
    L.ipkgpu_max_k.argtypes = [C.c_uint32]
    for name in ("ipkgpu_score_groups", "ipkgpu_score_groups_device"):
        fn = getattr(L, name)
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u32p, C.c_uint32,
                       C.c_float, C.POINTER(C.c_void_p)]
    L.ipkgpu_result_num_groups.restype = C.c_uint32
    L.ipkgpu_result_num_groups.argtypes = [C.c_void_p]
    L.ipkgpu_result_group_ids.restype = u32p
    L.ipkgpu_result_group_ids.argtypes = [C.c_void_p]
    L.ipkgpu_result_offsets.restype = u64p
    L.ipkgpu_result_offsets.argtypes = [C.c_void_p]
    L.ipkgpu_result_emitted.restype = C.c_uint64
    L.ipkgpu_result_emitted.argtypes = [C.c_void_p]
    L.ipkgpu_result_keys.restype = u32p
    L.ipkgpu_result_keys.argtypes = [C.c_void_p]
    L.ipkgpu_result_scores.restype = f32p
    L.ipkgpu_result_scores.argtypes = [C.c_void_p]
    L.ipkgpu_result_keys_device.restype = C.c_void_p
    L.ipkgpu_result_keys_device.argtypes = [C.c_void_p]
    L.ipkgpu_result_scores_device.restype = C.c_void_p
    L.ipkgpu_result_scores_device.argtypes = [C.c_void_p]
    L.ipkgpu_result_time_ms.restype = C.c_double
    L.ipkgpu_result_time_ms.argtypes = [C.c_void_p, C.c_int]
    L.ipkgpu_result_free.restype = None
    L.ipkgpu_result_free.argtypes = [C.c_void_p]
    L.ipkgpu_score_groups_positions.restype = C.c_int
    L.ipkgpu_score_groups_positions.argtypes = L.ipkgpu_score_groups.argtypes
    L.ipkgpu_result_positions.restype = u32p
    L.ipkgpu_result_positions.argtypes = [C.c_void_p]
    _lib = L
    return L


def log_threshold(omega, sigma, k):
    return float(load_library().ipkgpu_log_threshold(C.c_float(omega), sigma, k))


def bits_per_symbol(sigma):
    return int(load_library().ipkgpu_bits_per_symbol(sigma))


def score_threshold(omega, sigma, k):
    L = load_library()
    _bind_keymajor(L)
    return float(L.ipkgpu_score_threshold(C.c_float(omega), sigma, k))


def kmer_batch(key, n_ranges):
    return int(load_library().ipkgpu_kmer_batch(key, n_ranges))


def max_k(sigma):
    """Largest k one call over the whole key space accepts (DNA 14, AA 6)."""
    return int(load_library().ipkgpu_max_k(sigma))


def max_k_keyrange(sigma):
    """Largest k buildable in key-range passes (DNA 16: u32 keys; AA: max_k)."""
    L = load_library()
    L.ipkgpu_max_k_keyrange.restype = C.c_uint32
    L.ipkgpu_max_k_keyrange.argtypes = [C.c_uint32]
    return int(L.ipkgpu_max_k_keyrange(sigma))


class Result:
    """Owner of an ipkgpu_result (CSR of per-branch (key, score) sets)."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle
        n = lib.ipkgpu_result_num_groups(handle)
        self.group_ids = np.ctypeslib.as_array(lib.ipkgpu_result_group_ids(handle), shape=(n,)).copy() if n else np.zeros(0, np.uint32)
        self.offsets = np.ctypeslib.as_array(lib.ipkgpu_result_offsets(handle), shape=(n + 1,)).copy()
        self.emitted = int(lib.ipkgpu_result_emitted(handle))

    @property
    def num_entries(self):
        return int(self.offsets[-1])

    def time_ms(self, which):
        return float(self._lib.ipkgpu_result_time_ms(self._h, which))

    def keys(self):
        n = self.num_entries
        if n == 0:
            return np.zeros(0, np.uint32)
        p = self._lib.ipkgpu_result_keys(self._h)
        if not p:
            raise IpkGpuError(2, "device-to-host copy of keys failed")
        return np.ctypeslib.as_array(p, shape=(n,))

    def scores(self):
        n = self.num_entries
        if n == 0:
            return np.zeros(0, np.float32)
        p = self._lib.ipkgpu_result_scores(self._h)
        if not p:
            raise IpkGpuError(2, "device-to-host copy of scores failed")
        return np.ctypeslib.as_array(p, shape=(n,))

    def positions(self):
        """Window positions aligned with keys()/scores() (KEEP_POSITIONS results only)."""
        n = self.num_entries
        if n == 0:
            return np.zeros(0, np.uint32)
        p = self._lib.ipkgpu_result_positions(self._h)
        if not p:
            raise IpkGpuError(1, "this result carries no positions")
        return np.ctypeslib.as_array(p, shape=(n,))

    def keys_device_ptr(self):
        return self._lib.ipkgpu_result_keys_device(self._h)

    def scores_device_ptr(self):
        return self._lib.ipkgpu_result_scores_device(self._h)

    def group(self, i):
        """(keys, scores) of the i-th group in first-seen order (host copies)."""
        a, b = int(self.offsets[i]), int(self.offsets[i + 1])
        return self.keys()[a:b], self.scores()[a:b]

    def free(self):
        if self._h:
            self._lib.ipkgpu_result_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    """One scoring context on one GPU (one process per GPU)."""

    def __init__(self, device_id=0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.ipkgpu_create(device_id, C.byref(h))
        if rc != 0:
            raise IpkGpuError(rc, self._lib.ipkgpu_last_error(None).decode())
        self._h = h
        self.device_id = device_id

    def _err(self, rc):
        return IpkGpuError(rc, self._lib.ipkgpu_last_error(self._h).decode())

    def last_tables_compressed(self):
        return bool(self._lib.ipkgpu_last_tables_compressed(self._h))

    def last_main_kernel(self):
        return self._lib.ipkgpu_last_main_kernel(self._h).decode()

    def set_option(self, name, value):
        """ipkgpu_set_option; "slice_long_lists" = 1: DNA k >= 13 windows whose half lists exceed the big-list kernels' capacity are scored
        in slices instead of failing the call (default 0)."""
        rc = self._lib.ipkgpu_set_option(self._h, name.encode(), int(value))
        if rc != 0:
            raise self._err(rc)

    def score_groups(self, logp, mat_group, k, log_eps, sigma=None, sites=None, n_mats=None):
        """logp: numpy float32 [n_mats, sites, sigma] (host path) or a torch CUDA tensor / raw
        device pointer with explicit n_mats/sites/sigma (device path)."""
        mat_group = np.ascontiguousarray(mat_group, dtype=np.uint32)
        out = C.c_void_p()
        gp = mat_group.ctypes.data_as(C.POINTER(C.c_uint32))
        if isinstance(logp, np.ndarray):
            logp = np.ascontiguousarray(logp, dtype=np.float32)
            n_mats, sites, sigma = logp.shape
            if mat_group.shape != (n_mats,):
                raise ValueError("mat_group must have one branch id per matrix")
            rc = self._lib.ipkgpu_score_groups(self._h, logp.ctypes.data_as(C.c_void_p), n_mats, sites, sigma,
                                               gp, k, C.c_float(log_eps), C.byref(out))
        else:
            if hasattr(logp, "data_ptr"):
                if not logp.is_cuda or not logp.is_contiguous() or logp.dtype.itemsize != 4:
                    raise ValueError("device path needs a contiguous float32 CUDA tensor")
                n_mats, sites, sigma = logp.shape
                ptr = logp.data_ptr()
                # the library works on its own stream: whatever produced `logp` on torch's stream must be complete
                import torch
                torch.cuda.current_stream().synchronize()
            else:
                ptr = int(logp)
            if mat_group.shape != (n_mats,):
                raise ValueError("mat_group must have one branch id per matrix")
            rc = self._lib.ipkgpu_score_groups_device(self._h, C.c_void_p(ptr), n_mats, sites, sigma,
                                                      gp, k, C.c_float(log_eps), C.byref(out))
        if rc != 0:
            raise self._err(rc)
        return self._adopt(Result(self._lib, out))

    def score_groups_positions(self, logp, mat_group, k, log_eps):
        """KEEP_POSITIONS flavour (ipk-aa-pos): logp numpy float32 [n_mats, sites, sigma]; Result.positions()."""
        logp = np.ascontiguousarray(logp, dtype=np.float32)
        mat_group = np.ascontiguousarray(mat_group, dtype=np.uint32)
        n_mats, sites, sigma = logp.shape
        if mat_group.shape != (n_mats,):
            raise ValueError("mat_group must have one branch id per matrix")
        out = C.c_void_p()
        rc = self._lib.ipkgpu_score_groups_positions(self._h, logp.ctypes.data_as(C.c_void_p), n_mats, sites, sigma,
                                                     mat_group.ctypes.data_as(C.POINTER(C.c_uint32)), k, C.c_float(log_eps),
                                                     C.byref(out))
        if rc != 0:
            raise self._err(rc)
        return self._adopt(Result(self._lib, out))

    def _adopt(self, obj):
        """Results, parts and databases hold device blocks of this context: close() frees the ones still alive first (a handle freed
        after its context is a crash, and a failing test leaves exactly that order to the garbage collector)."""
        kids = self.__dict__.setdefault("_children", weakref.WeakSet())
        kids.add(obj)
        return obj

    def close(self):
        if self._h:
            for kid in list(self.__dict__.get("_children", ())):
                try:
                    kid.free()
                except Exception:
                    pass
            self._lib.ipkgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- key-major parts / database shards (multi-GPU exchange step) ---------------------------------

class DiffCounts(C.Structure):
    """ipkgpu_db_diff_counts (include/ipkgpu.h)"""
    _fields_ = [(n, C.c_uint64) for n in ("keys_a", "keys_b", "keys_only_a", "keys_only_b", "entries_a", "entries_b", "entries_only_a",
                                          "entries_only_b", "scores_differ", "positions_differ")] + [("max_abs_diff", C.c_double)]


# ipkgpu_db_diff_record: a difference of two databases; a score of NaN = not scored there
DIFF_RECORD = np.dtype([("key", "<u4"), ("branch", "<u4"), ("a_score", "<f4"), ("b_score", "<f4")])


def _bind_keymajor(L):
    if getattr(L, "_km_bound", False):
        return
    u32p, u64p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)
    L.ipkgpu_score_groups_keymajor_device.restype = C.c_int
    L.ipkgpu_score_groups_keymajor_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u32p,
                                                      C.c_uint32, C.c_float, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ipkgpu_score_groups_keyrange_device.restype = C.c_int
    L.ipkgpu_score_groups_keyrange_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, u32p,
                                                      C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ipkgpu_score_groups_keymajor_positions_device.restype = C.c_int
    L.ipkgpu_score_groups_keymajor_positions_device.argtypes = L.ipkgpu_score_groups_keymajor_device.argtypes
    L.ipkgpu_score_groups_keymajor_positions_owners_device.restype = C.c_int
    L.ipkgpu_score_groups_keymajor_positions_owners_device.argtypes = L.ipkgpu_score_groups_keymajor_device.argtypes
    L.ipkgpu_parts_positions_device.restype = C.c_void_p
    L.ipkgpu_parts_positions_device.argtypes = [C.c_void_p]
    L.ipkgpu_db_positions.restype = u32p
    L.ipkgpu_db_positions.argtypes = [C.c_void_p]
    L.ipkgpu_db_positions_device.restype = C.c_void_p
    L.ipkgpu_db_positions_device.argtypes = [C.c_void_p]
    L.ipkgpu_parts_key_base.restype = C.c_uint64
    L.ipkgpu_parts_key_base.argtypes = [C.c_void_p]
    L.ipkgpu_parts_num_owners.restype = C.c_uint32
    L.ipkgpu_parts_num_owners.argtypes = [C.c_void_p]
    L.ipkgpu_parts_slots.restype = C.c_uint64
    L.ipkgpu_parts_slots.argtypes = [C.c_void_p]
    L.ipkgpu_parts_counts_device.restype = C.c_void_p
    L.ipkgpu_parts_counts_device.argtypes = [C.c_void_p]
    L.ipkgpu_parts_entries_device.restype = C.c_void_p
    L.ipkgpu_parts_entries_device.argtypes = [C.c_void_p]
    L.ipkgpu_parts_owner_offsets.restype = u64p
    L.ipkgpu_parts_owner_offsets.argtypes = [C.c_void_p]
    L.ipkgpu_parts_emitted.restype = C.c_uint64
    L.ipkgpu_parts_emitted.argtypes = [C.c_void_p]
    L.ipkgpu_parts_time_ms.restype = C.c_double
    L.ipkgpu_parts_time_ms.argtypes = [C.c_void_p, C.c_int]
    L.ipkgpu_parts_free.restype = None
    L.ipkgpu_parts_free.argtypes = [C.c_void_p]
    L.ipkgpu_merge_parts.restype = C.c_int
    L.ipkgpu_merge_parts.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                     C.c_void_p, C.c_void_p, u64p, C.POINTER(C.c_void_p)]
    L.ipkgpu_merge_parts_ptrs.restype = C.c_int
    L.ipkgpu_merge_parts_ptrs.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.ipkgpu_merge_parts_positions_ptrs.restype = C.c_int
    L.ipkgpu_merge_parts_positions_ptrs.argtypes = L.ipkgpu_merge_parts_ptrs.argtypes[:-1] + [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]
    L.ipkgpu_comm_unique_id.restype = C.c_int
    L.ipkgpu_comm_unique_id.argtypes = [C.c_void_p]
    L.ipkgpu_comm_init.restype = C.c_int
    L.ipkgpu_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.ipkgpu_comm_available.restype = C.c_int
    L.ipkgpu_comm_available.argtypes = []
    L.ipkgpu_comm_prepare.restype = C.c_int
    L.ipkgpu_comm_prepare.argtypes = [C.c_void_p, C.c_int]
    for n in ("ipkgpu_comm_rank", "ipkgpu_comm_world"):
        getattr(L, n).restype = C.c_int
        getattr(L, n).argtypes = [C.c_void_p]
    L.ipkgpu_exchange_begin.restype = C.c_int
    L.ipkgpu_exchange_begin.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.ipkgpu_exchange_merge.restype = C.c_int
    L.ipkgpu_exchange_merge.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p),
                                        C.POINTER(C.c_double)]
    L.ipkgpu_xfer_exposed_ms.restype = C.c_double
    L.ipkgpu_xfer_exposed_ms.argtypes = [C.c_void_p]
    L.ipkgpu_xfer_free.restype = None
    L.ipkgpu_xfer_free.argtypes = [C.c_void_p]
    L.ipkgpu_db_from_parts.restype = C.c_int
    L.ipkgpu_db_from_parts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_num_keys.restype = C.c_uint64
    L.ipkgpu_db_num_keys.argtypes = [C.c_void_p]
    L.ipkgpu_db_num_entries.restype = C.c_uint64
    L.ipkgpu_db_num_entries.argtypes = [C.c_void_p]
    L.ipkgpu_db_keys.restype = u32p
    L.ipkgpu_db_keys.argtypes = [C.c_void_p]
    L.ipkgpu_db_key_offsets.restype = u64p
    L.ipkgpu_db_key_offsets.argtypes = [C.c_void_p]
    L.ipkgpu_db_entries.restype = u32p
    L.ipkgpu_db_entries.argtypes = [C.c_void_p]
    for n in ("ipkgpu_db_keys_device", "ipkgpu_db_key_offsets_device", "ipkgpu_db_entries_device"):
        getattr(L, n).restype = C.c_void_p
        getattr(L, n).argtypes = [C.c_void_p]
    L.ipkgpu_db_time_ms.restype = C.c_double
    L.ipkgpu_db_time_ms.argtypes = [C.c_void_p]
    L.ipkgpu_db_free.restype = None
    L.ipkgpu_db_free.argtypes = [C.c_void_p]
    L.ipkgpu_score_threshold.restype = C.c_float
    L.ipkgpu_score_threshold.argtypes = [C.c_float, C.c_uint32, C.c_uint32]
    L.ipkgpu_db_filter_mif0.restype = C.c_int
    L.ipkgpu_db_filter_mif0.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float]
    L.ipkgpu_db_filter_random.restype = C.c_int
    L.ipkgpu_db_filter_random.argtypes = [C.c_void_p, C.c_void_p]
    L.ipkgpu_db_filter_values.restype = C.POINTER(C.c_float)
    L.ipkgpu_db_filter_values.argtypes = [C.c_void_p]
    L.ipkgpu_db_filter_values_f64.restype = C.POINTER(C.c_double)
    L.ipkgpu_db_filter_values_f64.argtypes = [C.c_void_p]
    L.ipkgpu_db_filter_order.restype = u32p
    L.ipkgpu_db_filter_order.argtypes = [C.c_void_p]
    for n in ("ipkgpu_db_filter_values_device", "ipkgpu_db_filter_order_device"):
        getattr(L, n).restype = C.c_void_p
        getattr(L, n).argtypes = [C.c_void_p]
    L.ipkgpu_db_filter_time_ms.restype = C.c_double
    L.ipkgpu_db_filter_time_ms.argtypes = [C.c_void_p]
    L.ipkgpu_parts_spill.restype = C.c_int
    L.ipkgpu_parts_spill.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_uint32, u64p]
    L.ipkgpu_spill_merge.restype = C.c_int
    L.ipkgpu_spill_merge.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_char_p), C.c_uint32,
                                     C.POINTER(C.c_void_p)]
    L.ipkgpu_mem_stats.restype = C.c_int
    L.ipkgpu_mem_stats.argtypes = [C.c_void_p, u64p, u64p, C.c_int]
    L.ipkgpu_get_option.restype = C.c_int
    L.ipkgpu_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
    L.ipkgpu_db_load.restype = C.c_int
    L.ipkgpu_db_load.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_header_of.restype = C.c_void_p
    L.ipkgpu_db_header_of.argtypes = [C.c_void_p]
    L.ipkgpu_db_load_time.restype = C.c_double
    L.ipkgpu_db_load_time.argtypes = [C.c_void_p, C.c_int]
    L.ipkgpu_db_select.restype = C.c_int
    L.ipkgpu_db_select.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_float, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_load_select.restype = C.c_int
    L.ipkgpu_db_load_select.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_float, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_select_time_ms.restype = C.c_double
    L.ipkgpu_db_select_time_ms.argtypes = [C.c_void_p]
    L.ipkgpu_db_mu_kmers.restype = C.c_uint64
    L.ipkgpu_db_mu_kmers.argtypes = [C.c_double, C.c_uint64]
    L.ipkgpu_db_diff.restype = C.c_int
    L.ipkgpu_db_diff.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.POINTER(DiffCounts), C.c_void_p, C.c_uint64, u64p]
    L.ipkgpu_db_diff_time_ms.restype = C.c_double
    L.ipkgpu_db_diff_time_ms.argtypes = [C.c_void_p]
    L.ipkgpu_db_diff_chunk.restype = C.c_uint32
    L.ipkgpu_db_diff_chunk.argtypes = []
    L._km_bound = True


ABI_SYMBOLS += [
    "ipkgpu_score_groups_keymajor_device", "ipkgpu_parts_num_owners", "ipkgpu_parts_slots",
    "ipkgpu_parts_counts_device", "ipkgpu_parts_entries_device", "ipkgpu_parts_owner_offsets",
    "ipkgpu_parts_emitted", "ipkgpu_parts_time_ms", "ipkgpu_parts_free", "ipkgpu_merge_parts",
    "ipkgpu_db_num_keys", "ipkgpu_db_num_entries", "ipkgpu_db_keys", "ipkgpu_db_key_offsets", "ipkgpu_db_entries",
    "ipkgpu_db_keys_device", "ipkgpu_db_key_offsets_device", "ipkgpu_db_entries_device", "ipkgpu_db_time_ms",
    "ipkgpu_db_free", "ipkgpu_db_from_parts",
    "ipkgpu_score_threshold", "ipkgpu_db_filter_mif0", "ipkgpu_db_filter_values", "ipkgpu_db_filter_values_f64",
    "ipkgpu_db_filter_order", "ipkgpu_db_filter_values_device", "ipkgpu_db_filter_order_device",
    "ipkgpu_db_filter_time_ms",
    "ipkgpu_merge_parts_ptrs", "ipkgpu_comm_unique_id", "ipkgpu_comm_init", "ipkgpu_comm_rank", "ipkgpu_comm_world",
    "ipkgpu_exchange_begin", "ipkgpu_exchange_merge", "ipkgpu_xfer_exposed_ms", "ipkgpu_xfer_free",
    "ipkgpu_comm_available", "ipkgpu_comm_prepare",
    "ipkgpu_max_k_keyrange", "ipkgpu_score_groups_keyrange_device", "ipkgpu_parts_key_base",
    "ipkgpu_score_groups_keymajor_positions_device", "ipkgpu_parts_positions_device", "ipkgpu_db_positions",
    "ipkgpu_db_positions_device",
    "ipkgpu_score_groups_keymajor_positions_owners_device", "ipkgpu_merge_parts_positions_ptrs",
    "ipkgpu_parts_spill", "ipkgpu_spill_merge", "ipkgpu_mem_stats", "ipkgpu_get_option",
    "ipkgpu_db_filter_random",
    "ipkgpu_db_load", "ipkgpu_db_header_of", "ipkgpu_db_load_time", "ipkgpu_db_diff", "ipkgpu_db_diff_time_ms", "ipkgpu_db_diff_chunk",
    "ipkgpu_db_select", "ipkgpu_db_load_select", "ipkgpu_db_select_time_ms", "ipkgpu_db_mu_kmers",
]


class Parts:
    """This rank's key-major partial database, split by owner (device resident)."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle
        self.n_owners = int(lib.ipkgpu_parts_num_owners(handle))
        self.slots = int(lib.ipkgpu_parts_slots(handle))
        self.owner_offsets = np.ctypeslib.as_array(lib.ipkgpu_parts_owner_offsets(handle), shape=(self.n_owners + 1,)).copy()
        self.emitted = int(lib.ipkgpu_parts_emitted(handle))
        self.key_base = int(lib.ipkgpu_parts_key_base(handle))      # key-range parts: slot q is key key_base + q
        self.extra_ms = {}        # timings of further pieces folded into this object (distributed.build_db_shard)

    @property
    def num_entries(self):
        return int(self.owner_offsets[-1])

    def counts_ptr(self):
        return self._lib.ipkgpu_parts_counts_device(self._h)

    def entries_ptr(self):
        return self._lib.ipkgpu_parts_entries_device(self._h)

    def time_ms(self, which):
        return float(self._lib.ipkgpu_parts_time_ms(self._h, which)) + self.extra_ms.get(which, 0.0)

    def counts_tensor(self):
        """torch view [n_owners, slots] int32 of the device counts (keeps self alive)."""
        return _device_tensor(self.counts_ptr(), (self.n_owners, self.slots), "int32", self)

    def entries_tensor(self):
        """torch view [num_entries, 2] int32 (branch, score bits)."""
        return _device_tensor(self.entries_ptr(), (max(self.num_entries, 0), 2), "int32", self)

    def positions_ptr(self):
        """Device pointer of the entries' window starts; None for parts of a call without positions."""
        return self._lib.ipkgpu_parts_positions_device(self._h)

    def positions_tensor(self):
        """torch view [num_entries] int32 of the window starts, aligned with entries_tensor (score_groups_keymajor_positions)."""
        p = self.positions_ptr()
        if not p:
            raise IpkGpuError(1, "these parts carry no positions")
        return _device_tensor(p, (max(self.num_entries, 0),), "int32", self)

    def free(self):
        if self._h:
            self._lib.ipkgpu_parts_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Db:
    """One owner's shard of the phylo-k-mer database: key -> [(branch, score)] in reference order."""

    header = None          # Engine.load_db: the head of the file the database was loaded from (dbfile.file_info's dict)
    omega = None           # Engine.select_db / load_db with omega=: the omega the selection was made at (Engine.place's default threshold)

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle
        self.num_keys = int(lib.ipkgpu_db_num_keys(handle))
        self.num_entries = int(lib.ipkgpu_db_num_entries(handle))

    def time_ms(self):
        return float(self._lib.ipkgpu_db_time_ms(self._h))

    def keys(self):
        if self.num_keys == 0:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(self._lib.ipkgpu_db_keys(self._h), shape=(self.num_keys,))

    def key_offsets(self):
        return np.ctypeslib.as_array(self._lib.ipkgpu_db_key_offsets(self._h), shape=(self.num_keys + 1,))

    def entries(self):
        """(branches u32 [n], scores f32 [n])"""
        if self.num_entries == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.float32)
        e = np.ctypeslib.as_array(self._lib.ipkgpu_db_entries(self._h), shape=(self.num_entries, 2))
        return e[:, 0].copy(), e[:, 1].copy().view(np.float32)

    def positions(self):
        """Window starts u32 [n] aligned with entries(); None for a database without positions."""
        if not self._lib.ipkgpu_db_positions_device(self._h):
            return None
        if self.num_entries == 0:
            return np.zeros(0, np.uint32)
        return np.ctypeslib.as_array(self._lib.ipkgpu_db_positions(self._h), shape=(self.num_entries,))

    def positions_device_ptr(self):
        return self._lib.ipkgpu_db_positions_device(self._h)

    def filter_mif0(self, engine, total_num_groups, threshold):
        """MIF0 filter values + k-mer order (filter.cpp:55-119, db_builder.cpp:281-284) on the device."""
        rc = self._lib.ipkgpu_db_filter_mif0(engine._h, self._h, int(total_num_groups), C.c_float(threshold))
        if rc != 0:
            raise engine._err(rc)

    def filter_random(self, engine):
        """The random filter on the device: dbfile.splitmix_unit of every key as the filter value, and the k-mer order."""
        rc = self._lib.ipkgpu_db_filter_random(engine._h, self._h)
        if rc != 0:
            raise engine._err(rc)

    def filter_values(self, f64=False):
        n = self.num_keys
        if n == 0:
            return np.zeros(0, np.float64 if f64 else np.float32)
        p = (self._lib.ipkgpu_db_filter_values_f64 if f64 else self._lib.ipkgpu_db_filter_values)(self._h)
        if not p:
            raise IpkGpuError(1, "filter values not computed")
        return np.ctypeslib.as_array(p, shape=(n,))

    def filter_order(self):
        n = self.num_keys
        if n == 0:
            return np.zeros(0, np.uint32)
        p = self._lib.ipkgpu_db_filter_order(self._h)
        if not p:
            raise IpkGpuError(1, "filter order not computed")
        return np.ctypeslib.as_array(p, shape=(n,))

    def filter_time_ms(self):
        return float(self._lib.ipkgpu_db_filter_time_ms(self._h))

    def keys_device_ptr(self):
        return self._lib.ipkgpu_db_keys_device(self._h)

    def key_offsets_device_ptr(self):
        return self._lib.ipkgpu_db_key_offsets_device(self._h)

    def entries_device_ptr(self):
        return self._lib.ipkgpu_db_entries_device(self._h)

    def free(self):
        if self._h:
            self._lib.ipkgpu_db_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _device_tensor(ptr, shape, dtype, owner):
    """Zero-copy torch view of engine-owned device memory via __cuda_array_interface__."""
    import torch

    n = int(np.prod(shape))
    if n == 0 or not ptr:
        return torch.empty(shape, dtype=getattr(torch, dtype), device="cuda")

    class _Holder:
        pass
    h = _Holder()
    h.__cuda_array_interface__ = {"shape": tuple(int(x) for x in shape), "typestr": "<i4", "data": (int(ptr), False),
                                  "version": 3, "strides": None}
    h._owner = owner
    t = torch.as_tensor(h, device="cuda")
    t._ipk_owner = owner
    return t


def _score_groups_keymajor(self, logp, mat_group, k, log_eps, n_owners=1, sigma=None, sites=None, n_mats=None, keyrange=None,
                           positions=False, owners=False):
    """Scoring pass with key-major, owner-split output (see include/ipkgpu.h). logp: torch CUDA tensor
    [n_mats, sites, sigma] float32 or a raw device pointer with explicit shape.  keyrange = (lead, cls): the key-range pass of
    the k-mers whose first `lead` symbols spell `cls` (one owner; ipkgpu_score_groups_keyrange_device)."""
    _bind_keymajor(self._lib)
    mat_group = np.ascontiguousarray(mat_group, dtype=np.uint32)
    keep = None
    if isinstance(logp, np.ndarray):
        import torch
        keep = torch.from_numpy(np.ascontiguousarray(logp, dtype=np.float32)).cuda()
        logp = keep
    if hasattr(logp, "data_ptr"):
        if not logp.is_cuda or not logp.is_contiguous() or logp.dtype.itemsize != 4:
            raise ValueError("device path needs a contiguous float32 CUDA tensor")
        n_mats, sites, sigma = logp.shape
        ptr = logp.data_ptr() if n_mats else 0
        import torch
        st = torch.cuda.current_stream()
        if not st.query():                     # whatever produced logp on torch's stream must be done (the engine has its own stream)
            st.synchronize()
    else:
        ptr = int(logp)
    out = C.c_void_p()
    if keyrange is not None:
        lead, cls = keyrange
        rc = self._lib.ipkgpu_score_groups_keyrange_device(self._h, C.c_void_p(ptr), n_mats, sites, sigma,
                                                           mat_group.ctypes.data_as(C.POINTER(C.c_uint32)), k,
                                                           C.c_float(log_eps), lead, cls, C.byref(out))
    elif positions:
        call = self._lib.ipkgpu_score_groups_keymajor_positions_owners_device if owners else self._lib.ipkgpu_score_groups_keymajor_positions_device
        rc = call(self._h, C.c_void_p(ptr), n_mats, sites, sigma,
                                                                     mat_group.ctypes.data_as(C.POINTER(C.c_uint32)), k,
                                                                     C.c_float(log_eps), n_owners, C.byref(out))
    else:
        rc = self._lib.ipkgpu_score_groups_keymajor_device(self._h, C.c_void_p(ptr), n_mats, sites, sigma,
                                                           mat_group.ctypes.data_as(C.POINTER(C.c_uint32)), k,
                                                           C.c_float(log_eps), n_owners, C.byref(out))
    del keep
    if rc != 0:
        raise self._err(rc)
    return self._adopt(Parts(self._lib, out))


def _merge_parts(self, sigma, k, owner, n_owners, counts, entries, source_offsets):
    """counts: device tensor/pointer u32 [n_sources, slots]; entries: device tensor/pointer [n, 2];
    source_offsets: entry offset of each source's block inside `entries` (host, length n_sources)."""
    _bind_keymajor(self._lib)
    so = np.ascontiguousarray(source_offsets, dtype=np.uint64)
    cp = counts.data_ptr() if hasattr(counts, "data_ptr") else int(counts)
    ep = entries.data_ptr() if hasattr(entries, "data_ptr") else int(entries or 0)
    out = C.c_void_p()
    rc = self._lib.ipkgpu_merge_parts(self._h, sigma, k, owner, n_owners, len(so), C.c_void_p(cp), C.c_void_p(ep),
                                      so.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return self._adopt(Db(self._lib, out))


def _merge_parts_ptrs(self, sigma, k, owner, n_owners, counts_ptrs, entries_ptrs):
    """One (counts row, entry block) device pointer pair per source, in source order."""
    _bind_keymajor(self._lib)
    n = len(counts_ptrs)
    cp = (C.c_void_p * n)(*[int(x) for x in counts_ptrs])
    ep = (C.c_void_p * n)(*[int(x) for x in entries_ptrs])
    out = C.c_void_p()
    rc = self._lib.ipkgpu_merge_parts_ptrs(self._h, sigma, k, owner, n_owners, n, cp, ep, C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return self._adopt(Db(self._lib, out))


def _merge_parts_positions_ptrs(self, sigma, k, owner, n_owners, counts_ptrs, entries_ptrs, positions_ptrs):
    """merge_parts_ptrs over positioned sources: one (counts row, entry block, window starts) device pointer triple per source, in
    source order; the Db has positions()."""
    _bind_keymajor(self._lib)
    n = len(counts_ptrs)
    if len(entries_ptrs) != n or len(positions_ptrs) != n:
        raise ValueError("one counts, entries and positions pointer per source")
    cp = (C.c_void_p * n)(*[int(x) for x in counts_ptrs])
    ep = (C.c_void_p * n)(*[int(x) for x in entries_ptrs])
    pp = (C.c_void_p * n)(*[int(x) for x in positions_ptrs])
    out = C.c_void_p()
    rc = self._lib.ipkgpu_merge_parts_positions_ptrs(self._h, sigma, k, owner, n_owners, n, cp, ep, pp, C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return self._adopt(Db(self._lib, out))


def _comm_unique_id(self):
    _bind_keymajor(self._lib)
    buf = (C.c_uint8 * 128)()
    rc = self._lib.ipkgpu_comm_unique_id(buf)
    if rc != 0:
        raise IpkGpuError(rc, self._lib.ipkgpu_last_error(None).decode())
    return bytes(buf)


def _comm_prepare(self, world):
    """The local half of the communicator set-up (RCCL loaded, exchange stream and size buffers allocated): everything that
    can fail on one rank alone, done before the collective comm_init so that the ranks can agree on it first."""
    _bind_keymajor(self._lib)
    rc = self._lib.ipkgpu_comm_prepare(self._h, world)
    if rc != 0:
        raise self._err(rc)


def _comm_world_seen(self):
    """World size of the library's RCCL communicator (1 without one): what RCCL itself was initialised with."""
    _bind_keymajor(self._lib)
    return int(self._lib.ipkgpu_comm_world(self._h))


def _comm_init(self, unique_id, rank, world):
    """RCCL communicator of this context (the id's 128 bytes come from rank 0's comm_unique_id)."""
    _bind_keymajor(self._lib)
    buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
    rc = self._lib.ipkgpu_comm_init(self._h, buf, rank, world)
    if rc != 0:
        raise self._err(rc)
    self.comm_world, self.comm_rank = world, rank


def _exchange_begin(self, parts):
    """Enqueues block o -> rank o of one piece; positioned parts send their window starts beside the entries."""
    out = C.c_void_p()
    rc = self._lib.ipkgpu_exchange_begin(self._h, parts._h, C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return out


def _exchange_merge(self, xfers, sigma, k):
    """-> (Db, exposed transfer time in ms); frees the transfer handles.  All pieces positioned: the Db has positions(); a mixture of
    positioned and plain pieces is refused."""
    n = len(xfers)
    arr = (C.c_void_p * n)(*[x.value for x in xfers])
    out = C.c_void_p()
    exposed = C.c_double(0.0)
    rc = self._lib.ipkgpu_exchange_merge(self._h, arr, n, sigma, k, C.byref(out), C.byref(exposed))
    for x in xfers:
        self._lib.ipkgpu_xfer_free(x)
    if rc != 0:
        raise self._err(rc)
    return self._adopt(Db(self._lib, out)), float(exposed.value)


def _db_from_parts(self, parts, sigma, k):
    """Single-owner parts -> database without copying the entries (they move into the Db)."""
    _bind_keymajor(self._lib)
    out = C.c_void_p()
    rc = self._lib.ipkgpu_db_from_parts(self._h, parts._h, sigma, k, C.byref(out))
    if rc != 0:
        raise self._err(rc)
    parts.owner_offsets = parts.owner_offsets.copy()
    return self._adopt(Db(self._lib, out))


Engine.db_from_parts = _db_from_parts
Engine.merge_parts_ptrs = _merge_parts_ptrs
Engine.merge_parts_positions_ptrs = _merge_parts_positions_ptrs
Engine.comm_unique_id = _comm_unique_id
Engine.comm_init = _comm_init
Engine.comm_prepare = _comm_prepare
Engine.comm_world_seen = _comm_world_seen
Engine.exchange_begin = _exchange_begin
Engine.exchange_merge = _exchange_merge
Engine.comm_world = 1
Engine.comm_rank = 0
Engine.score_groups_keymajor = _score_groups_keymajor


def _score_groups_keyrange(self, logp, mat_group, k, log_eps, lead, cls):
    """Key-range pass: Parts of the k-mers whose first `lead` symbols spell `cls` (base sigma), key_base set
    (include/ipkgpu.h, ipkgpu_score_groups_keyrange_device).  logp as for score_groups_keymajor."""
    return _score_groups_keymajor(self, logp, mat_group, k, log_eps, keyrange=(int(lead), int(cls)))


Engine.score_groups_keyrange = _score_groups_keyrange


def _score_groups_keymajor_positions(self, logp, mat_group, k, log_eps, n_owners=1, sigma=None, sites=None, n_mats=None):
    """score_groups_keymajor with every entry's window start riding along (Parts.positions_tensor, Db.positions): one scoring
    pass on the device (include/ipkgpu.h, ipkgpu_score_groups_keymajor_positions_device).  One owner only."""
    return _score_groups_keymajor(self, logp, mat_group, k, log_eps, n_owners=n_owners, sigma=sigma, sites=sites, n_mats=n_mats,
                                  positions=True)


Engine.score_groups_keymajor_positions = _score_groups_keymajor_positions


def _score_groups_keymajor_positions_owners(self, logp, mat_group, k, log_eps, n_owners=1, sigma=None, sites=None, n_mats=None):
    """score_groups_keymajor_positions split by owner (include/ipkgpu.h, ipkgpu_score_groups_keymajor_positions_owners_device): any
    n_owners >= 1, block o of Parts.positions_tensor() beside block o of the entries; no matrices give empty positioned parts."""
    return _score_groups_keymajor(self, logp, mat_group, k, log_eps, n_owners=n_owners, sigma=sigma, sites=sites, n_mats=n_mats,
                                  positions=True, owners=True)


Engine.score_groups_keymajor_positions_owners = _score_groups_keymajor_positions_owners
Engine.merge_parts = _merge_parts


def _parts_spill(self, parts, directory, piece):
    """Packs and writes every owner block of `parts` as directory/p<piece>_b<owner>.blk (include/ipkgpu.h, ipkgpu_parts_spill);
    returns the bytes written."""
    _bind_keymajor(self._lib)
    n = C.c_uint64(0)
    rc = self._lib.ipkgpu_parts_spill(self._h, parts._h, os.fsencode(directory), int(piece), C.byref(n))
    if rc != 0:
        raise self._err(rc)
    return int(n.value)


def _spill_merge(self, sigma, k, owner, n_owners, block_paths):
    """One batch's database out of its spill blocks, read in the order given = piece order (ipkgpu_spill_merge)."""
    _bind_keymajor(self._lib)
    n = len(block_paths)
    arr = (C.c_char_p * n)(*[os.fsencode(p) for p in block_paths])
    out = C.c_void_p()
    rc = self._lib.ipkgpu_spill_merge(self._h, sigma, k, owner, n_owners, arr, n, C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return self._adopt(Db(self._lib, out))


def _mem_stats(self, reset_peak=False):
    """(held, held_peak): bytes of device memory the context holds from hipMalloc, and their high-water mark (ipkgpu_mem_stats)."""
    _bind_keymajor(self._lib)
    held, peak = C.c_uint64(0), C.c_uint64(0)
    rc = self._lib.ipkgpu_mem_stats(self._h, C.byref(held), C.byref(peak), 1 if reset_peak else 0)
    if rc != 0:
        raise self._err(rc)
    return int(held.value), int(peak.value)


def _get_option(self, name):
    """"workspace_bytes", "device_budget_bytes", "last_refused_bytes", "slice_long_lists", "debug_sliced_windows" (the windows
    scored in slices by this engine so far) or "debug_pool_bytes" (bytes the pair pool holds) (ipkgpu_get_option)."""
    _bind_keymajor(self._lib)
    v = C.c_int64(0)
    rc = self._lib.ipkgpu_get_option(self._h, name.encode(), C.byref(v))
    if rc != 0:
        raise IpkGpuError(rc, f"no readable option '{name}'")
    return int(v.value)


Engine.get_option = _get_option
Engine.parts_spill = _parts_spill
Engine.spill_merge = _spill_merge
Engine.mem_stats = _mem_stats


def mu_kmers(mu, n_kmers):
    """ipkgpu_db_mu_kmers: the number of k-mers the fraction mu of n_kmers stands for, min(n, ceil(mu * n)) in binary64 (no GPU needed).
    mu outside [0, 1] or NaN is refused here."""
    mu = float(mu)
    if not 0.0 <= mu <= 1.0:
        raise ValueError(f"mu must be in [0, 1], not {mu}")
    L = load_library()
    _bind_keymajor(L)
    return int(L.ipkgpu_db_mu_kmers(mu, int(n_kmers)))


def _selection_args(header, n_kmers, keep_kmers, mu, min_log_score, omega):
    """(M, t) of a selection from one of keep_kmers / mu and one of min_log_score / omega (none of a pair: all k-mers, every entry)."""
    if keep_kmers is not None and mu is not None:
        raise ValueError("give keep_kmers or mu, not both")
    if min_log_score is not None and omega is not None:
        raise ValueError("give min_log_score or omega, not both")
    m = (1 << 64) - 1 if keep_kmers is None else int(keep_kmers)
    if mu is not None:
        m = mu_kmers(mu, n_kmers)
    if m < 0:
        raise ValueError("keep_kmers must not be negative")
    t = -np.inf if min_log_score is None else float(min_log_score)
    if omega is not None:
        if header is None:
            raise ValueError("omega= needs a database loaded from a file (sigma and k come from its head); give min_log_score")
        # in binary32, the type the file stores its omega in and ipkgpu_log_threshold takes: the build's own decimal (1.7) is not below 1.70000005
        if not np.float32(omega) >= np.float32(header["omega"]):
            raise ValueError(f"omega {omega} is below the file's omega {header['omega']}: entries under the build's threshold are not in the file")
        sigma = {"DNA": 4, "AA": 20}.get(header["sequence_type"], 0)
        t = log_threshold(float(omega), sigma, int(header["kmer_size"]))
    return min(m, (1 << 64) - 1), t


def _finish_selection(self, out, omega):
    from . import dbfile
    db = self._adopt(Db(self._lib, out))
    head = self._lib.ipkgpu_db_header_of(out)
    db.header = dbfile.info_of_handle(head) if head else None
    db.omega = None if omega is None else float(omega)
    return db


def _select_db(self, db, keep_kmers=None, mu=None, min_log_score=None, omega=None, wanted=None):
    """ipkgpu_db_select: the first keep_kmers k-mers of `db` in filter order (or its fraction mu: mu_kmers), of those the entries with
    score > min_log_score (or above log_threshold(omega, sigma, k) of the database's head) -- a new, ordinary Db; `db` is untouched.
    The definition is in include/ipkgpu.h and is this library's own.  A selection made with omega= remembers it (`.omega`): Engine.place
    then takes that omega's threshold by default.  `.header` is the source's with the totals replaced (its omega is not changed)."""
    _bind_keymajor(self._lib)
    if wanted is not None:
        return _select_wanted(self, db, keep_kmers, mu, min_log_score, omega, wanted)
    m, t = _selection_args(db.header, db.num_keys, keep_kmers, mu, min_log_score, omega)
    out = C.c_void_p()
    rc = self._lib.ipkgpu_db_select(self._h, db._h, m, C.c_float(t), C.byref(out))
    if rc != 0:
        raise self._err(rc)
    sel = _finish_selection(self, out, omega if omega is not None else db.omega)
    if sel.header is None and db.header is not None:
        # a union of files (load_dbs) has no file behind it: its head is the shard set's, kept on the Python side alone
        sel.header = dict(db.header, total_num_kmers=sel.num_keys, total_num_entries=sel.num_entries)
    return sel


def _select_time_ms(self):
    """Device time of the engine's last selection (ipkgpu_db_select_time_ms)."""
    _bind_keymajor(self._lib)
    return float(self._lib.ipkgpu_db_select_time_ms(self._h))


def _load_db(self, path, mu=None, omega=None, keep_kmers=None, min_log_score=None, wanted=None, key_range=None):
    """ipkgpu_db_load: a database file onto the device -- the Db the builds produce, with the file's filter values and record order
    (filter_values(), filter_order()) and `.header`, the dict dbfile.read_db returns for the file's head.
    dbfile.write_db_device(engine, db, path, **dbfile.header_args(db.header)) gives the file back byte for byte.
    With mu, omega, keep_kmers or min_log_score: ipkgpu_db_load_select -- select_db(load_db(path), ...) array for array, reading only the
    prefix of the file that holds the first k-mers asked for (mu counts against the header's total).
    With wanted= (a KmerSet of Engine.kmer_set): ipkgpu_db_load_wanted -- select_db(load_db(path, ...), wanted=wanted) array for array, the
    file streamed through a device window of option "db_load_window_bytes" and never held whole: for a file larger than device memory.
    With key_range=(lo, hi): ipkgpu_db_load_key_range -- the records with lo <= key < hi (hi at most 2^32), every one with all its entries,
    through the same streamed load; no other selection goes with it."""
    from . import dbfile
    _bind_keymajor(self._lib)
    out = C.c_void_p()
    if key_range is not None:
        if wanted is not None or mu is not None or omega is not None or keep_kmers is not None or min_log_score is not None:
            raise ValueError("key_range= goes with no other selection")
        _bind_diff_files(self._lib)
        lo, hi = (int(x) for x in key_range)
        if lo < 0 or hi < 0 or hi >= 1 << 64:
            raise ValueError("key_range is (lo, hi) with 0 <= lo <= hi <= 2^32")
        rc = self._lib.ipkgpu_db_load_key_range(self._h, os.fsencode(path), lo, hi, C.byref(out))
        if rc != 0:
            raise self._err(rc)
        return _finish_selection(self, out, None)
    if wanted is not None:
        _bind_stream(self._lib)
        head = dbfile.file_info(path)
        m, t = _selection_args(head, head["total_num_kmers"], keep_kmers, mu, min_log_score, omega)
        rc = self._lib.ipkgpu_db_load_wanted(self._h, os.fsencode(path), wanted._h, m, C.c_float(t), C.byref(out))
        if rc != 0:
            raise self._err(rc)
        return _finish_selection(self, out, omega)
    if mu is None and omega is None and keep_kmers is None and min_log_score is None:
        rc = self._lib.ipkgpu_db_load(self._h, os.fsencode(path), C.byref(out))
        if rc != 0:
            raise self._err(rc)
        db = self._adopt(Db(self._lib, out))
        db.header = dbfile.info_of_handle(self._lib.ipkgpu_db_header_of(out))
        return db
    head = dbfile.file_info(path)
    m, t = _selection_args(head, head["total_num_kmers"], keep_kmers, mu, min_log_score, omega)
    rc = self._lib.ipkgpu_db_load_select(self._h, os.fsencode(path), m, C.c_float(t), C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return _finish_selection(self, out, omega)


def _load_times(self):
    """The engine's last load_db: seconds in all / reading the file / in the host's walk / waiting for the device, and milliseconds of
    db_unpack_heads_kernel, db_unpack_entries_kernel and of all device work behind the last copy; the body bytes read; and for a
    load with wanted= the number of windows and the records kept (ipkgpu_db_load_time)."""
    _bind_keymajor(self._lib)
    names = ("total_s", "read_s", "walk_s", "device_wait_s", "heads_ms", "entries_ms", "device_ms", "body_bytes_read", "windows", "records_kept")
    return {k: float(self._lib.ipkgpu_db_load_time(self._h, i)) for i, k in enumerate(names)}


def _diff_dbs(self, a, b, eps=1e-2, max_records=0):
    """ipkgpu_db_diff: the reference's ipkdiff comparison (tools/src/diff.cpp:210-295) of two databases of this engine on the device.
    Returns (counts dict, records): records = the first max_records differences as a DIFF_RECORD array (ascending key; inside a key
    A's entries in A's order, then B's unmatched ones in B's order; NaN = not scored).  eps = 0: the score bits must be equal."""
    _bind_keymajor(self._lib)
    counts = DiffCounts()
    rec = np.zeros(max(int(max_records), 1), DIFF_RECORD)
    n = C.c_uint64(0)
    rc = self._lib.ipkgpu_db_diff(self._h, a._h, b._h, float(eps), C.byref(counts), rec.ctypes.data, int(max_records), C.byref(n))
    if rc != 0:
        raise self._err(rc)
    d = {name: int(getattr(counts, name)) for name, _ in DiffCounts._fields_[:-1]}
    d["max_abs_diff"] = float(counts.max_abs_diff)
    return d, rec[:int(n.value)].copy()


def _diff_time_ms(self):
    _bind_keymajor(self._lib)
    return float(self._lib.ipkgpu_db_diff_time_ms(self._h))


# ---- two files compared by key ranges (ipkgpu_db_diff_files) ---------------------------------------------------------------------------

ABI_SYMBOLS += [
    "ipkgpu_db_load_key_range", "ipkgpu_db_diff_files", "ipkgpu_db_diff_files_num_ranges", "ipkgpu_db_diff_files_range",
    "ipkgpu_db_diff_files_stat", "ipkgpu_db_diff_files_range_bytes", "ipkgpu_db_stream_window_bytes",
]

DIFF_FILES_STATS = ("total_s", "hist_s", "loads_s", "diff_ms", "body_bytes_read", "passes_a", "passes_b", "walk_s", "window_bytes", "avail_bytes",
                    "max_window_records", "longest_record_bytes")


def _bind_diff_files(L):
    if getattr(L, "_diff_files_bound", False):
        return
    L.ipkgpu_db_load_key_range.restype = C.c_int
    L.ipkgpu_db_load_key_range.argtypes = [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_diff_files.restype = C.c_int
    L.ipkgpu_db_diff_files.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_double, C.POINTER(DiffCounts), C.c_void_p, C.c_uint64,
                                       C.POINTER(C.c_uint64)]
    L.ipkgpu_db_diff_files_num_ranges.restype = C.c_uint64
    L.ipkgpu_db_diff_files_num_ranges.argtypes = [C.c_void_p]
    L.ipkgpu_db_diff_files_range.restype = C.c_int
    L.ipkgpu_db_diff_files_range.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ipkgpu_db_diff_files_stat.restype = C.c_double
    L.ipkgpu_db_diff_files_stat.argtypes = [C.c_void_p, C.c_int]
    L.ipkgpu_db_diff_files_range_bytes.restype = C.c_uint64
    L.ipkgpu_db_diff_files_range_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64]
    L.ipkgpu_db_stream_window_bytes.restype = C.c_uint64
    L.ipkgpu_db_stream_window_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64]
    L._diff_files_bound = True


def stream_window_bytes(window, n_w, longest):
    """ipkgpu_db_stream_window_bytes: the fixed device bytes of one file's streamed passes (the formula of include/ipkgpu.h; no GPU)."""
    L = load_library()
    _bind_diff_files(L)
    return int(L.ipkgpu_db_stream_window_bytes(int(window), int(n_w), int(longest)))


def diff_files_range_bytes(fixed, n_a, e_a, positioned_a, n_b, e_b, positioned_b, max_records=0):
    """ipkgpu_db_diff_files_range_bytes: the peak device bytes of comparing one key range (the formula of include/ipkgpu.h; no GPU)."""
    L = load_library()
    _bind_diff_files(L)
    return int(L.ipkgpu_db_diff_files_range_bytes(int(fixed), int(n_a), int(e_a), int(bool(positioned_a)), int(n_b), int(e_b), int(bool(positioned_b)),
                                                  int(max_records)))


def _diff_files_info(self):
    """The engine's last diff_files: "ranges" [(lo, hi)] and the figures of DIFF_FILES_STATS (ipkgpu_db_diff_files_stat)."""
    _bind_diff_files(self._lib)
    info = {k: float(self._lib.ipkgpu_db_diff_files_stat(self._h, i)) for i, k in enumerate(DIFF_FILES_STATS)}
    for k in DIFF_FILES_STATS[4:7] + DIFF_FILES_STATS[8:]:
        info[k] = int(info[k])
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    info["ranges"] = []
    for i in range(int(self._lib.ipkgpu_db_diff_files_num_ranges(self._h))):
        self._lib.ipkgpu_db_diff_files_range(self._h, i, C.byref(lo), C.byref(hi))
        info["ranges"].append((int(lo.value), int(hi.value)))
    return info


def _diff_files(self, a, b, eps=1e-2, max_records=0):
    """ipkgpu_db_diff_files: diff_dbs(load_db(a), load_db(b), eps, max_records) field for field, for files that do not fit device memory
    together -- compared by key ranges planned against "device_budget_bytes" (or the device's free memory).  Returns (counts, records,
    info); info: _diff_files_info's dict (the ranges, the passes over each body, seconds and bytes)."""
    _bind_keymajor(self._lib)
    _bind_diff_files(self._lib)
    counts = DiffCounts()
    rec = np.zeros(max(int(max_records), 1), DIFF_RECORD)
    n = C.c_uint64(0)
    rc = self._lib.ipkgpu_db_diff_files(self._h, os.fsencode(a), os.fsencode(b), float(eps), C.byref(counts), rec.ctypes.data, int(max_records),
                                        C.byref(n))
    if rc != 0:
        raise self._err(rc)
    d = {name: int(getattr(counts, name)) for name, _ in DiffCounts._fields_[:-1]}
    d["max_abs_diff"] = float(counts.max_abs_diff)
    return d, rec[:int(n.value)].copy(), _diff_files_info(self)


Engine.diff_files = _diff_files
Engine.diff_files_info = _diff_files_info
Engine.load_db = _load_db
Engine.select_db = _select_db
Engine.select_time_ms = _select_time_ms
Engine.load_times = _load_times
Engine.diff_dbs = _diff_dbs
Engine.diff_time_ms = _diff_time_ms


# ---- placement: query sequences on a database of this engine (ipkgpu_db_place) ------------------------------------------------

ABI_SYMBOLS += [
    "ipkgpu_db_place", "ipkgpu_placements_num_queries", "ipkgpu_placements_keep", "ipkgpu_placements_branches",
    "ipkgpu_placements_scores", "ipkgpu_placements_counts", "ipkgpu_placements_lwr", "ipkgpu_placements_n_kmers",
    "ipkgpu_placements_n_found", "ipkgpu_placements_n_branches", "ipkgpu_placements_time_ms", "ipkgpu_placements_free",
    "ipkgpu_db_place_opts", "ipkgpu_placements_strand", "ipkgpu_placements_n_ambiguous",
]

PLACE_NONE = 0xFFFFFFFF      # the branch past a query's last placement


class _PlaceOptions(C.Structure):
    _fields_ = [("ambiguity", C.c_uint32), ("strands", C.c_uint32)]


def _bind_place(L):
    if getattr(L, "_place_bound", False):
        return
    L.ipkgpu_db_place.restype = C.c_int
    L.ipkgpu_db_place.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64,
                                  C.c_uint32, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_place_opts.restype = C.c_int
    L.ipkgpu_db_place_opts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p, C.c_uint64,
                                       C.c_uint32, C.POINTER(_PlaceOptions), C.POINTER(C.c_void_p)]
    L.ipkgpu_placements_num_queries.restype = C.c_uint64
    L.ipkgpu_placements_keep.restype = C.c_uint32
    for name, t in (("branches", C.c_uint32), ("scores", C.c_float), ("counts", C.c_uint32), ("lwr", C.c_double), ("n_kmers", C.c_uint32),
                    ("n_found", C.c_uint32), ("n_branches", C.c_uint32), ("strand", C.c_uint8), ("n_ambiguous", C.c_uint32)):
        getattr(L, "ipkgpu_placements_" + name).restype = C.POINTER(t)
    for name in ("num_queries", "keep", "branches", "scores", "counts", "lwr", "n_kmers", "n_found", "n_branches", "strand", "n_ambiguous", "free"):
        getattr(L, "ipkgpu_placements_" + name).argtypes = [C.c_void_p]
    L.ipkgpu_placements_time_ms.restype = C.c_double
    L.ipkgpu_placements_time_ms.argtypes = [C.c_void_p, C.c_int]
    L.ipkgpu_placements_free.restype = None
    L._place_bound = True


class Placements:
    """Host arrays of one Engine.place call: branches u32 / scores f32 / counts u32 / lwr f64, each [n, keep] and best first (past a
    query's last placement: branch PLACE_NONE, zeros); n_kmers / n_found / n_branches u32 [n]; strand u8 [n] (0: the strand given,
    1: the reverse complement was placed) and n_ambiguous u32 [n] (expanded windows), both zero without the options of Engine.place;
    time_ms: total (host clock), index (the database's first call only) and place (the placement kernels)."""

    def __init__(self, lib, h):
        n, keep = int(lib.ipkgpu_placements_num_queries(h)), int(lib.ipkgpu_placements_keep(h))
        self.n, self.keep = n, keep

        def arr(name, dtype, shape):
            if n == 0:
                return np.zeros(shape, dtype)
            return np.ctypeslib.as_array(getattr(lib, "ipkgpu_placements_" + name)(h), shape=shape).astype(dtype, copy=True)
        self.branches = arr("branches", np.uint32, (n, keep))
        self.scores = arr("scores", np.float32, (n, keep))
        self.counts = arr("counts", np.uint32, (n, keep))
        self.lwr = arr("lwr", np.float64, (n, keep))
        self.n_kmers = arr("n_kmers", np.uint32, (n,))
        self.n_found = arr("n_found", np.uint32, (n,))
        self.n_branches = arr("n_branches", np.uint32, (n,))
        self.strand = arr("strand", np.uint8, (n,))
        self.n_ambiguous = arr("n_ambiguous", np.uint32, (n,))
        self.time_ms = {k: float(lib.ipkgpu_placements_time_ms(h, i)) for i, k in enumerate(("total", "index", "place"))}


def _place_packed(self, db, blob, offsets, keep_at_most=7, sigma=None, k=None, log_eps=None, ambiguity=False, strands="given"):
    """Engine.place over packed queries: `blob` (bytes or a uint8 array) holds query i at [offsets[i], offsets[i + 1])."""
    if strands not in ("given", "both"):
        raise ValueError('strands is "given" or "both"')
    _bind_keymajor(self._lib)
    _bind_place(self._lib)
    h = db.header
    if sigma is None or k is None or log_eps is None:
        if h is None:
            raise ValueError("sigma, k and log_eps are needed for a database that was not loaded from a file")
        sigma = {"DNA": 4, "AA": 20}.get(h["sequence_type"], 0) if sigma is None else sigma
        k = h["kmer_size"] if k is None else k
        log_eps = log_threshold(h["omega"] if db.omega is None else db.omega, sigma, k) if log_eps is None else log_eps
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if len(off) < 1:
        raise ValueError("offsets needs one element more than there are queries")
    data = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else np.ascontiguousarray(blob, dtype=np.uint8)
    if len(off) > 1 and int(off.max()) > len(data):
        raise ValueError("an offset points past the end of the sequences")
    out = C.c_void_p()
    if ambiguity or strands == "both":
        opts = _PlaceOptions(int(bool(ambiguity)), int(strands == "both"))
        rc = self._lib.ipkgpu_db_place_opts(self._h, db._h, int(sigma), int(k), C.c_float(log_eps), data.ctypes.data, off.ctypes.data,
                                            len(off) - 1, int(keep_at_most), C.byref(opts), C.byref(out))
    else:
        rc = self._lib.ipkgpu_db_place(self._h, db._h, int(sigma), int(k), C.c_float(log_eps), data.ctypes.data, off.ctypes.data, len(off) - 1,
                                       int(keep_at_most), C.byref(out))
    if rc != 0:
        raise self._err(rc)
    try:
        return Placements(self._lib, out)
    finally:
        self._lib.ipkgpu_placements_free(out)


def _place(self, db, seqs, keep_at_most=7, sigma=None, k=None, log_eps=None, ambiguity=False, strands="given"):
    """ipkgpu_db_place: places the query sequences `seqs` (str or bytes each) on the database `db` of this engine -> Placements.
    sigma, k and log_eps default to those of the file a loaded database came from (its header's sequence type, k-mer size and
    log_threshold(omega, sigma, k)); a database built in this process needs them given.
    ambiguity=True expands a window with one ambiguous symbol (N, R, Y, ...; amino acids B, Z, J, X) into its resolutions;
    strands="both" places the reverse complement as well (DNA) and keeps the better strand (ipkgpu_db_place_opts in include/ipkgpu.h)."""
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        off[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
    return _place_packed(self, db, b"".join(raw), off, keep_at_most, sigma, k, log_eps, ambiguity, strands)


Engine.place_packed = _place_packed
Engine.place = _place


# ---- placing on a file that does not fit device memory: the queries' k-mer set, the restriction, the streamed load -----------------

ABI_SYMBOLS += [
    "ipkgpu_kmer_set_of_queries", "ipkgpu_kmer_set_count", "ipkgpu_kmer_set_num_words", "ipkgpu_kmer_set_words", "ipkgpu_kmer_set_sigma",
    "ipkgpu_kmer_set_k", "ipkgpu_kmer_set_free", "ipkgpu_db_select_keys", "ipkgpu_db_load_wanted",
]

ERR_NOMEM = 3


def _bind_stream(L):
    if getattr(L, "_stream_bound", False):
        return
    _bind_place(L)
    L.ipkgpu_kmer_set_of_queries.restype = C.c_int
    L.ipkgpu_kmer_set_of_queries.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(_PlaceOptions),
                                             C.POINTER(C.c_void_p)]
    L.ipkgpu_kmer_set_count.restype = C.c_uint64
    L.ipkgpu_kmer_set_num_words.restype = C.c_uint64
    L.ipkgpu_kmer_set_words.restype = C.POINTER(C.c_uint32)
    L.ipkgpu_kmer_set_sigma.restype = C.c_uint32
    L.ipkgpu_kmer_set_k.restype = C.c_uint32
    L.ipkgpu_kmer_set_free.restype = None
    for name in ("count", "num_words", "words", "sigma", "k", "free"):
        getattr(L, "ipkgpu_kmer_set_" + name).argtypes = [C.c_void_p]
    L.ipkgpu_db_select_keys.restype = C.c_int
    L.ipkgpu_db_select_keys.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_load_wanted.restype = C.c_int
    L.ipkgpu_db_load_wanted.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_float, C.POINTER(C.c_void_p)]
    L._stream_bound = True


class KmerSet:
    """The k-mer set of a batch of queries (ipkgpu_kmer_set_of_queries): a bitmap over the code space on the device.  count: the distinct
    codes; words(): a host copy of the bitmap, bit `code` of 32-bit word code >> 5."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle
        self.count = int(lib.ipkgpu_kmer_set_count(handle))
        self.sigma, self.k = int(lib.ipkgpu_kmer_set_sigma(handle)), int(lib.ipkgpu_kmer_set_k(handle))

    def words(self):
        n = int(self._lib.ipkgpu_kmer_set_num_words(self._h))
        p = self._lib.ipkgpu_kmer_set_words(self._h)
        if not p:
            raise MemoryError("no host copy of the k-mer set")
        return np.ctypeslib.as_array(p, shape=(n,)).copy()

    def free(self):
        if self._h:
            self._lib.ipkgpu_kmer_set_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _pack(seqs):
    raw = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    off = np.zeros(len(raw) + 1, np.uint64)
    if raw:
        off[1:] = np.cumsum([len(r) for r in raw], dtype=np.uint64)
    return np.frombuffer(b"".join(raw), np.uint8), off


def _kmer_set(self, seqs, sigma, k, ambiguity=False, strands="given"):
    """ipkgpu_kmer_set_of_queries: every k-mer code Engine.place(db, seqs, ambiguity=, strands=) would look up -> KmerSet.
    A database restricted to it (select_db / load_db with wanted=) places `seqs` bit for bit as the whole database does."""
    if strands not in ("given", "both"):
        raise ValueError('strands is "given" or "both"')
    _bind_keymajor(self._lib)
    _bind_stream(self._lib)
    data, off = _pack(seqs)
    opts = _PlaceOptions(int(bool(ambiguity)), int(strands == "both"))
    out = C.c_void_p()
    rc = self._lib.ipkgpu_kmer_set_of_queries(self._h, int(sigma), int(k), data.ctypes.data, off.ctypes.data, len(off) - 1, C.byref(opts), C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return self._adopt(KmerSet(self._lib, out))


def _select_wanted(self, db, keep_kmers, mu, min_log_score, omega, wanted):
    """select_db(db, ..., wanted=set): the selection, if one is asked for, then its restriction to the set (ipkgpu_db_select_keys)."""
    _bind_stream(self._lib)
    src = db
    if not (keep_kmers is None and mu is None and min_log_score is None and omega is None):
        src = _select_db(self, db, keep_kmers, mu, min_log_score, omega)
    try:
        out = C.c_void_p()
        rc = self._lib.ipkgpu_db_select_keys(self._h, src._h, wanted._h, C.byref(out))
        if rc != 0:
            raise self._err(rc)
        return _finish_selection(self, out, src.omega)
    finally:
        if src is not db:
            src.free()


def _place_file(self, path, seqs, keep_at_most=7, ambiguity=False, strands="given", mu=None, omega=None, query_batch=None):
    """Places `seqs` on the database FILE `path` without ever holding the file on the device: for each batch of query_batch queries
    (None: all at once) the batch's k-mer set, the streamed load of the records it names (load_db(path, mu=, omega=, wanted=set)), the
    placement, and both freed -> one Placements over all queries, equal to place(load_db(path, mu=, omega=), seqs, ...).
    A batch whose restricted database does not fit (IPKGPU_ERR_NOMEM) is retried in halves, down to one query; then the error stands."""
    from . import dbfile
    seqs = list(seqs)
    head = dbfile.file_info(path)
    sigma = {"DNA": 4, "AA": 20}.get(head["sequence_type"], 0)
    k = int(head["kmer_size"])
    step = len(seqs) if query_batch is None else int(query_batch)
    if query_batch is not None and step < 1:
        raise ValueError("query_batch must be at least 1")
    parts = []

    def run(batch):
        try:
            kset = self.kmer_set(batch, sigma, k, ambiguity, strands)
            try:
                db = self.load_db(path, mu=mu, omega=omega, wanted=kset)
                try:
                    parts.append(self.place(db, batch, keep_at_most, ambiguity=ambiguity, strands=strands))
                finally:
                    db.free()
            finally:
                kset.free()
        except IpkGpuError as e:
            if e.code != ERR_NOMEM or len(batch) < 2:
                raise
            half = (len(batch) + 1) // 2
            run(batch[:half])
            run(batch[half:])

    for i in range(0, len(seqs), max(step, 1)):
        run(seqs[i:i + step])
    if not parts:
        run([])
    return _concat_placements(parts)


def _concat_placements(parts):
    if len(parts) == 1:
        return parts[0]
    res = object.__new__(Placements)
    res.n, res.keep = sum(p.n for p in parts), parts[0].keep
    for name in ("branches", "scores", "counts", "lwr", "n_kmers", "n_found", "n_branches", "strand", "n_ambiguous"):
        setattr(res, name, np.concatenate([getattr(p, name) for p in parts]))
    res.time_ms = {key: sum(p.time_ms[key] for p in parts) for key in parts[0].time_ms}
    return res


Engine.kmer_set = _kmer_set
Engine.place_file = _place_file


# ---- the union of databases with disjoint key sets (ipkgpu_db_union) ----------------------------------------------------------------

ABI_SYMBOLS += ["ipkgpu_db_union", "ipkgpu_db_union_bytes", "ipkgpu_db_union_time_ms", "ipkgpu_db_union_files"]

UNION_TIMES = ("total_ms", "key_sort_ms", "entry_copy_ms", "order_sort_ms")


def _bind_union(L):
    if getattr(L, "_union_bound", False):
        return
    L.ipkgpu_db_union.restype = C.c_int
    L.ipkgpu_db_union.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_union_bytes.restype = C.c_uint64
    L.ipkgpu_db_union_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_int]
    L.ipkgpu_db_union_time_ms.restype = C.c_double
    L.ipkgpu_db_union_time_ms.argtypes = [C.c_void_p, C.c_int]
    L._union_bound = True


def union_bytes(n_keys, n_entries, n_srcs, positioned):
    """ipkgpu_db_union_bytes: the peak device bytes a union of n_srcs databases with n_keys keys and n_entries entries in all holds on
    top of its sources -- the result and the workspace (the formula of include/ipkgpu.h; no GPU)."""
    L = load_library()
    _bind_union(L)
    return int(L.ipkgpu_db_union_bytes(int(n_keys), int(n_entries), int(n_srcs), int(bool(positioned))))


def _union_dbs(self, dbs):
    """ipkgpu_db_union: the databases `dbs` of this engine, whose key sets are disjoint and which all carry filter values (loaded, or
    filtered), as ONE ordinary Db -- keys ascending, every key's entries, positions and filter values bit for bit its source's, the order
    by (filter value, key).  The sources are only read and stay valid.  `.header` is None."""
    _bind_keymajor(self._lib)
    _bind_union(self._lib)
    dbs = list(dbs)
    arr = (C.c_void_p * max(len(dbs), 1))(*[d._h for d in dbs])
    out = C.c_void_p()
    rc = self._lib.ipkgpu_db_union(self._h, arr, len(dbs), C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return self._adopt(Db(self._lib, out))


def _union_times(self):
    """Device milliseconds of the engine's last union: all, the key sort (sort keys to key offsets), the entry copy, the order sort."""
    _bind_union(self._lib)
    return {k: float(self._lib.ipkgpu_db_union_time_ms(self._h, i)) for i, k in enumerate(UNION_TIMES)}


def shard_set_head(infos, names):
    """The head a set of shard files stands for, from their file_info dicts: sequence type, k, omega and the positions flag must agree
    (ValueError naming the file that differs); the tree is the first non-empty newick's -- pass files and ranks' shards carry an empty
    one -- and two different non-empty trees are an error.  Returns header_args' dict plus "positions_loaded"."""
    if not infos:
        raise ValueError("no database file given")
    first = infos[0]
    tree = None
    for info, name in zip(infos, names):
        for field, what in (("sequence_type", "sequence type"), ("kmer_size", "k"), ("positions_loaded", "positions flag")):
            if info[field] != first[field]:
                raise ValueError(f"{name}: {what} {info[field]} differs from {names[0]}'s {first[field]}")
        if np.float32(info["omega"]).view(np.uint32) != np.float32(first["omega"]).view(np.uint32):
            raise ValueError(f"{name}: omega {info['omega']} differs from {names[0]}'s {first['omega']}")
        if info["newick"]:
            if tree is None:
                tree = (info, name)
            elif info["newick"] != tree[0]["newick"] or info["tree_index"] != tree[0]["tree_index"]:
                raise ValueError(f"{name}: its tree differs from {tree[1]}'s")
    src = tree[0] if tree else first
    return dict(sequence_type=first["sequence_type"], tree_index=src["tree_index"], newick=src["newick"], kmer_size=first["kmer_size"],
                omega=first["omega"], positions_loaded=first["positions_loaded"])


def _load_dbs(self, paths):
    """Several database files with disjoint key sets as one Db: each is loaded (load_db), the heads are checked to agree
    (shard_set_head), the databases are united (union_dbs) and the sources freed.  Returns (Db, head): head is shard_set_head's dict
    with the union's totals, and is also the Db's `.header`, so select_db(omega=) and place take the union like a loaded file."""
    paths = [os.fspath(p) for p in paths]
    srcs = []
    try:
        for p in paths:
            srcs.append(self.load_db(p))
        head = shard_set_head([d.header for d in srcs], paths)
        db = self.union_dbs(srcs)
    finally:
        for d in srcs:
            d.free()
    head.update(total_num_kmers=db.num_keys, total_num_entries=db.num_entries)
    db.header = head
    return db, head


Engine.union_dbs = _union_dbs
Engine.union_bytes = staticmethod(union_bytes)
Engine.union_times = _union_times
Engine.load_dbs = _load_dbs


# ---- the join of databases that share k-mers (ipkgpu_db_join) -----------------------------------------------------------------------

ABI_SYMBOLS += ["ipkgpu_db_join", "ipkgpu_db_join_bytes", "ipkgpu_db_join_stat"]

JOIN_STATS = ("total_ms", "key_ms", "entry_copy_ms", "duplicate_ms", "shared_keys", "entries_dropped", "route")


def _bind_join(L):
    if getattr(L, "_join_bound", False):
        return
    L.ipkgpu_db_join.restype = C.c_int
    L.ipkgpu_db_join.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]
    L.ipkgpu_db_join_bytes.restype = C.c_uint64
    L.ipkgpu_db_join_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_int]
    L.ipkgpu_db_join_stat.restype = C.c_double
    L.ipkgpu_db_join_stat.argtypes = [C.c_void_p, C.c_int]
    L._join_bound = True


def join_bytes(keys_in_all, entries_in_all, n_srcs, positioned):
    """ipkgpu_db_join_bytes: an upper bound of the device bytes a join of n_srcs databases with keys_in_all keys and entries_in_all
    entries in all (summed over the sources) holds on top of its sources (the formula of include/ipkgpu.h; no GPU)."""
    L = load_library()
    _bind_join(L)
    return int(L.ipkgpu_db_join_bytes(int(keys_in_all), int(entries_in_all), int(n_srcs), int(bool(positioned))))


def _join_dbs(self, dbs):
    """ipkgpu_db_join: the databases `dbs` of this engine, whose key sets may overlap, as ONE Db -- the set union of the keys,
    ascending; a key's entries are its sources' lists concatenated in the order of `dbs`, a branch that occurs again kept once at its
    first place with the reference's `put` maximum (a later score replaces only if strictly greater; its position goes with it).
    The sources need no filter values and stay valid.  The result has no filter values, no order and no header: filter it
    (Db.filter_mif0 / filter_random) before it is written or consumed."""
    _bind_keymajor(self._lib)
    _bind_join(self._lib)
    dbs = list(dbs)
    arr = (C.c_void_p * max(len(dbs), 1))(*[d._h for d in dbs])
    out = C.c_void_p()
    rc = self._lib.ipkgpu_db_join(self._h, arr, len(dbs), C.byref(out))
    if rc != 0:
        raise self._err(rc)
    return self._adopt(Db(self._lib, out))


def _join_stats(self):
    """The engine's last join: device milliseconds in all, in the key stage, the entry copy and the duplicate stage; the keys found in
    more than one source, the entries dropped as duplicates, the route taken (0 concatenation only, 1 duplicates resolved)."""
    _bind_join(self._lib)
    return {k: float(self._lib.ipkgpu_db_join_stat(self._h, i)) for i, k in enumerate(JOIN_STATS)}


Engine.join_dbs = _join_dbs
Engine.join_bytes = staticmethod(join_bytes)
Engine.join_stats = _join_stats


# ---- the join of branch shards that do not fit device memory, by key ranges (ipkgpu_db_join_files) -----------------------------------------

ABI_SYMBOLS += ["ipkgpu_db_join_files", "ipkgpu_db_join_files_range_bytes", "ipkgpu_db_join_files_num_ranges", "ipkgpu_db_join_files_range",
                "ipkgpu_db_join_files_stat"]

JOIN_FILES_STATS = ("total_s", "hist_s", "loads_s", "join_ms", "body_bytes_read", "passes", "walk_s", "write_s", "merge_s", "window_bytes", "avail_bytes",
                    "shared_keys", "entries_dropped", "route1_ranges", "range_peak_bytes")


def _bind_join_files(L):
    if getattr(L, "_join_files_bound", False):
        return
    from .dbfile import _Header
    L.ipkgpu_db_join_files.restype = C.c_int
    L.ipkgpu_db_join_files.argtypes = [C.c_void_p, C.POINTER(_Header), C.POINTER(C.c_char_p), C.c_uint32, C.c_int, C.c_uint64, C.c_float, C.c_char_p,
                                       C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ipkgpu_db_join_files_range_bytes.restype = C.c_uint64
    L.ipkgpu_db_join_files_range_bytes.argtypes = [C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_int, C.c_uint64, C.c_uint64]
    L.ipkgpu_db_join_files_num_ranges.restype = C.c_uint64
    L.ipkgpu_db_join_files_num_ranges.argtypes = [C.c_void_p]
    L.ipkgpu_db_join_files_range.restype = C.c_int
    L.ipkgpu_db_join_files_range.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.ipkgpu_db_join_files_stat.restype = C.c_double
    L.ipkgpu_db_join_files_stat.argtypes = [C.c_void_p, C.c_int]
    L._join_files_bound = True


def join_files_range_bytes(fixed, n, e, positioned, write_piece, longest_joined):
    """ipkgpu_db_join_files_range_bytes: the peak device bytes of joining, filtering and writing one key range of len(n) shards that hold
    n[s] records and e[s] entries in it (the formula of include/ipkgpu.h; no GPU)."""
    L = load_library()
    _bind_join_files(L)
    n, e = [int(x) for x in n], [int(x) for x in e]
    assert len(n) == len(e)
    arr = C.c_uint64 * max(len(n), 1)
    return int(L.ipkgpu_db_join_files_range_bytes(int(fixed), len(n), arr(*n), arr(*e), int(bool(positioned)), int(write_piece), int(longest_joined)))


def _join_files(self, paths, output, sequence_type, tree_index, newick, kmer_size, omega, filter_, n_nodes, threshold, tmp_dir=None):
    """ipkgpu_db_join_files: the file that loading `paths`, join_dbs in that order, the filter (filter_ "mif0" with n_nodes = MIF0's N of
    the WHOLE tree and the score threshold, or "random") and the device writer give, byte for byte, for shards that do not fit device
    memory together: joined by key ranges planned against "device_budget_bytes" (or the device's free memory), the range files merged
    on the host; tmp_dir (default: output + ".ranges") holds the range files meanwhile.  Returns (k-mers, entries, entries dropped)."""
    from .dbfile import _header
    if filter_ not in ("mif0", "random"):
        raise ValueError(f"unknown filter {filter_!r} (mif0, random)")
    _bind_keymajor(self._lib)
    _bind_join_files(self._lib)
    paths = [os.fspath(p) for p in paths]
    h = _header(sequence_type, tree_index, newick, kmer_size, omega)
    arr = (C.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])
    nk, ne, nd, nb = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = self._lib.ipkgpu_db_join_files(self._h, C.byref(h), arr, len(paths), 0 if filter_ == "mif0" else 1, int(n_nodes), float(threshold),
                                        os.fsencode(output), None if tmp_dir is None else os.fsencode(tmp_dir), C.byref(nk), C.byref(ne), C.byref(nd),
                                        C.byref(nb))
    if rc != 0:
        raise self._err(rc)
    return int(nk.value), int(ne.value), int(nd.value)


def _join_files_ranges(self):
    """[(lo, hi)] of the engine's last join_files."""
    _bind_join_files(self._lib)
    lo, hi = C.c_uint64(0), C.c_uint64(0)
    out = []
    for i in range(int(self._lib.ipkgpu_db_join_files_num_ranges(self._h))):
        self._lib.ipkgpu_db_join_files_range(self._h, i, C.byref(lo), C.byref(hi))
        out.append((int(lo.value), int(hi.value)))
    return out


def _join_files_stats(self):
    """The figures of JOIN_FILES_STATS for the engine's last join_files (ipkgpu_db_join_files_stat)."""
    _bind_join_files(self._lib)
    info = {k: float(self._lib.ipkgpu_db_join_files_stat(self._h, i)) for i, k in enumerate(JOIN_FILES_STATS)}
    for k in ("body_bytes_read", "passes") + JOIN_FILES_STATS[9:]:
        info[k] = int(info[k])
    return info


Engine.join_files = _join_files
Engine.join_files_ranges = _join_files_ranges
Engine.join_files_stats = _join_files_stats
Engine.join_files_range_bytes = staticmethod(join_files_range_bytes)
