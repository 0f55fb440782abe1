"""ctypes binding of libmhx.so (C ABI in include/mhx.h).

There is deliberately no fallback: if the HIP library is missing or no GPU is usable every
call raises.  The oracle under oracle/ is test infrastructure and is never imported here.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MHX_LIBRARY: load another build of the same library (the phase-timing debug build of tools/probe_phases.py)
LIB_PATH = os.environ.get("MHX_LIBRARY") or os.path.join(_HERE, "libmhx.so")

NUM_BUCKETS = 65536
MAX_MUL = 65535

BUF_EDGES = 1
BUF_BUCKET_COUNT = 2
BUF_FIRST_0_OUT = 3
BUF_LAST_0_IN = 4
BUF_MUL_HIST = 5
BUF_IS_SOLID = 6
BUF_MERCY_CAND = 7
BUF_SDBG_BYTES = 8
BUF_BUCKET_OFFSET = 9
BUF_BUCKET_TIPS = 10
BUF_BUCKET_LARGE = 11
BUF_SORTED_ITEMS = 12
(BUF_SDBG_W, BUF_SDBG_LAST, BUF_SDBG_TIP, BUF_SDBG_INVALID, BUF_SDBG_SMALL_MUL, BUF_SDBG_MUL, BUF_SDBG_TIP_LABELS, BUF_SDBG_PREFIX_LKT,
 BUF_SDBG_RS_W_L2, BUF_SDBG_RS_W_L1, BUF_SDBG_RS_W_SEL, BUF_SDBG_RS_LAST_L2, BUF_SDBG_RS_LAST_L1, BUF_SDBG_RS_LAST_SEL, BUF_SDBG_RS_TIP_L2,
 BUF_SDBG_RS_TIP_L1) = range(20, 36)
BUF_W_COUNT = 13
BUF_LIB_RECORDS = 40
BUF_UNITIG_VERTICES = 41
BUF_UNITIG_SEQ = 42
BUF_UNITIG_OFFSET = 43
BUF_UNITIG_BUBBLE_REC = 44
BUF_UNITIG_BUBBLE_SEQ = 45
BUF_LOCAL_REC = 46
BUF_LOCAL_ITEMS = 47
BUF_LOCAL_OFFSETS = 48
BUF_SDBG_MUL_HIST = 49
BUF_FASTX_TEXT = 50
SIM_MAX_LEN, SIM_MAX_INDEL = 16384, 2047
# one mhx_local_record (include/mhx.h)
LOCAL_RECORD_DTYPE = np.dtype([("contig_id", np.uint32), ("contig_from", np.int32), ("contig_to", np.int32), ("query_from", np.int32),
                               ("query_to", np.int32), ("mismatch", np.uint32), ("strand", np.uint32), ("valid", np.uint32)])
# one mhx_bubble_record (include/mhx.h)
BUBBLE_RECORD_DTYPE = np.dtype([("offset", np.uint64), ("length", np.uint32), ("vertex", np.uint32), ("avg_depth", np.float64)])
UNITIG_LOOP, UNITIG_PALINDROME, UNITIG_STANDALONE, UNITIG_CHANGED = 1, 2, 4, 8
# one mhx_unitig_vertex (include/mhx.h)
UNITIG_VERTEX_DTYPE = np.dtype([("b", np.uint64), ("e", np.uint64), ("rb", np.uint64), ("re", np.uint64), ("total_depth", np.uint64),
                                ("length", np.uint32), ("flags", np.uint32)])


class MhxError(RuntimeError):
    pass


class CountResult(C.Structure):
    _fields_ = [("n_items", C.c_uint64), ("n_distinct", C.c_uint64), ("n_edges", C.c_uint64),
                ("words_per_edge", C.c_uint32), ("item_words", C.c_uint32)]


class S1Result(C.Structure):
    _fields_ = [("n_items", C.c_uint64), ("n_solid", C.c_uint64), ("n_mercy_cand", C.c_uint64),
                ("item_words", C.c_uint32)]


class SdbgResult(C.Structure):
    _fields_ = [("n_items", C.c_uint64), ("n_sdbg", C.c_uint64), ("n_tips", C.c_uint64), ("n_large", C.c_uint64),
                ("sdbg_bytes", C.c_uint64), ("words_per_tip_label", C.c_uint32), ("item_words", C.c_uint32)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint32), ("total_ms", C.c_double),
                ("algo_bytes", C.c_double)]


class FastxResult(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_bases", C.c_uint64), ("n_words", C.c_uint64), ("max_len", C.c_uint32), ("status", C.c_int)]


class BgzfResult(C.Structure):
    _fields_ = [("status", C.c_int), ("reason", C.c_uint32), ("bad_block", C.c_uint64), ("n_blocks", C.c_uint64), ("n_text", C.c_uint64)]


class IterateResult(C.Structure):
    _fields_ = [("n_flanks", C.c_uint64), ("n_kmers", C.c_uint64), ("n_edges", C.c_uint64), ("words_per_edge", C.c_uint32)]


class SdbgIndexInfo(C.Structure):
    _fields_ = [("n_items", C.c_uint64), ("n_tips", C.c_uint64), ("n_large", C.c_uint64), ("k", C.c_uint32),
                ("words_per_tip_label", C.c_uint32), ("use_full_mul", C.c_int), ("num_l1_w", C.c_uint64), ("num_l2_w", C.c_uint64),
                ("num_l1_bits", C.c_uint64), ("num_l2_bits", C.c_uint64), ("w_char_count", C.c_uint64 * 9),
                ("w_sel_offset", C.c_uint64 * 10), ("ones_in_last", C.c_uint64), ("ones_in_tip", C.c_uint64),
                ("last_sel_count", C.c_uint64), ("f", C.c_longlong * 6), ("rank_f", C.c_longlong * 6)]


class UnitigResult(C.Structure):
    _fields_ = [("n_vertices", C.c_uint64), ("n_loops", C.c_uint64), ("n_palindromes", C.c_uint64), ("n_standalone", C.c_uint64),
                ("n_bases", C.c_uint64)]


class DistItems(C.Structure):
    _fields_ = [("d_items", C.c_void_p), ("n_items", C.c_uint64), ("item_bytes", C.c_uint32)]


STAGE_S1 = 1
STAGE_S2 = 2
STAGE_COUNT = 3
STAGE_SEQ2SDBG = 4
STAGE_S1_MERCY = 5

# every symbol include/mhx.h declares: (restype, argtypes)
_P = C.c_void_p
SYMBOLS = {
    "mhx_last_error": (C.c_char_p, []),
    "mhx_version": (C.c_char_p, []),
    "mhx_device_count": (C.c_int, []),
    "mhx_create": (_P, [C.c_int]),
    "mhx_destroy": (None, [_P]),
    "mhx_trim": (C.c_int, [_P]),
    "mhx_synchronize": (C.c_int, [_P]),
    "mhx_set_option": (C.c_int, [_P, C.c_char_p, C.c_longlong]),
    "mhx_get_option": (C.c_longlong, [_P, C.c_char_p, C.c_longlong]),
    "mhx_load_sequences": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint32, _P]),
    "mhx_load_bin_records": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_int]),
    "mhx_append_sequences": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint32, _P, _P]),
    "mhx_load_multiplicity": (C.c_int, [_P, _P, C.c_uint64]),
    "mhx_load_edges": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32]),
    "mhx_num_sequences": (C.c_uint64, [_P]),
    "mhx_fixed_length": (C.c_uint32, [_P]),
    "mhx_num_bases": (C.c_uint64, [_P]),
    "mhx_buffer_bytes": (C.c_uint64, [_P, C.c_int]),
    "mhx_fetch": (C.c_int, [_P, C.c_int, _P, C.c_uint64, C.c_uint64]),
    "mhx_count": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(CountResult)]),
    "mhx_read2sdbg_s1": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(S1Result)]),
    "mhx_read2sdbg_add_mercy": (C.c_int, [_P, C.c_uint32, C.POINTER(C.c_uint64)]),
    "mhx_set_is_solid": (C.c_int, [_P, _P, C.c_uint64]),
    "mhx_read2sdbg_s2": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.POINTER(SdbgResult)]),
    "mhx_seq2sdbg": (C.c_int, [_P, C.c_uint32, C.POINTER(SdbgResult)]),
    "mhx_gen_mercy_edges": (C.c_int, [_P, C.c_uint32, _P, C.c_uint64, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "mhx_sort_records": (C.c_int, [_P, _P, C.c_uint64, C.c_uint32, C.c_uint32]),
    "mhx_set_partition": (C.c_int, [_P, C.c_int, C.c_int, _P]),
    "mhx_set_global_layout": (C.c_int, [_P, C.c_uint64, C.c_uint64]),
    "mhx_dist_extract": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_uint32, C.POINTER(DistItems), _P]),
    "mhx_dist_recv_buffer": (_P, [_P, C.c_uint64, C.c_uint32]),
    "mhx_dist_process_s1": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(S1Result)]),
    "mhx_dist_process_s2": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(SdbgResult)]),
    "mhx_dist_process_count": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_uint64, C.POINTER(CountResult)]),
    "mhx_dist_process_seq2sdbg": (C.c_int, [_P, C.c_uint32, C.c_uint64, C.POINTER(SdbgResult)]),
    "mhx_dist_route_records": (C.c_int, [_P, C.c_int, C.c_uint64, C.POINTER(DistItems), _P]),
    "mhx_dist_apply_routed": (C.c_int, [_P, C.c_int, C.c_uint64]),
    "mhx_device_pointer": (_P, [_P, C.c_int]),
    "mhx_adopt_is_solid_slice": (C.c_int, [_P, _P, C.c_uint64]),
    "mhx_iterate": (C.c_int, [_P, C.c_uint32, C.c_uint32, _P, C.c_uint64, C.c_uint64, _P, C.POINTER(IterateResult)]),
    "mhx_local_index": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _P, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]),
    "mhx_local_map": (C.c_int, [_P, C.c_int32, C.c_double, C.POINTER(C.c_uint64)]),
    "mhx_local_insert_size": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                        C.POINTER(C.c_int32)]),
    "mhx_local_collect": (C.c_int, [_P, C.c_uint32, _P, _P, _P, _P, _P, _P]),
    "mhx_fastx_to_records": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(FastxResult)]),
    "mhx_bgzf_inflate": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.POINTER(BgzfResult)]),
    "mhx_fastx_bgzf_to_records": (C.c_int, [_P, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(FastxResult)]),
    "mhx_sdbg_build_index": (C.c_int, [_P, C.c_uint32, C.POINTER(SdbgIndexInfo)]),
    "mhx_sdbg_load_bytes": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, _P]),
    "mhx_sdbg_remove_tips": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.c_int, _P]),
    "mhx_sdbg_mul_histogram": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.POINTER(C.c_uint64)]),
    "mhx_infer_min_depth": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "mhx_sdbg_infer_min_depth": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "mhx_sdbg_unitigs": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.POINTER(UnitigResult)]),
    "mhx_unitig_disconnect_weak_links": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.c_double, C.POINTER(C.c_uint64)]),
    "mhx_unitig_remove_tips": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.c_uint32, C.POINTER(C.c_uint64)]),
    "mhx_unitig_remove_local_low_depth": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_int,
                                                    C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "mhx_unitig_iterate_local_low_depth": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.c_double, C.c_uint32, C.c_uint32, C.c_double, C.c_int,
                                                     C.POINTER(C.c_uint64)]),
    "mhx_unitig_finish": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.POINTER(UnitigResult)]),
    "mhx_unitig_pop_bubbles": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.c_uint32, C.c_double, C.c_double, C.c_int, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint64)]),
    "mhx_unitig_bubble_stats": (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    "mhx_unitig_remove_low_depth": (C.c_int, [_P, C.POINTER(SdbgIndexInfo), C.c_double, C.POINTER(C.c_uint64)]),
    "mhx_unitig_similarity": (C.c_int, [_P, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_double, C.POINTER(C.c_double)]),
    "mhx_comm_unique_id": (C.c_int, [_P]),
    "mhx_comm_init_rank": (_P, [_P, _P, C.c_int, C.c_int]),
    "mhx_comm_local_group": (C.c_int, [C.c_int, _P, _P]),
    "mhx_comm_destroy": (None, [_P]),
    "mhx_comm_rank": (C.c_int, [_P]),
    "mhx_comm_size": (C.c_int, [_P]),
    "mhx_comm_barrier": (C.c_int, [_P]),
    "mhx_comm_bytes_sent": (C.c_uint64, [_P, C.c_int]),
    "mhx_dist_plan_memory": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, C.c_int]),
    "mhx_comm_all_reduce_u64": (C.c_int, [_P, _P, C.c_uint64, C.c_int]),
    "mhx_dist_setup": (C.c_int, [_P, _P, C.c_int, C.c_uint32, C.c_uint32]),
    "mhx_dist_read2sdbg": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(S1Result), C.POINTER(SdbgResult), _P]),
    "mhx_dist_count": (C.c_int, [_P, _P, C.c_uint32, C.c_uint32, C.POINTER(CountResult)]),
    "mhx_dist_seq2sdbg": (C.c_int, [_P, _P, C.c_uint32, C.POINTER(SdbgResult)]),
    "mhx_dist_gen_mercy_edges": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, C.c_uint64, _P, C.POINTER(C.c_uint64)]),
    "mhx_device_free_bytes": (C.c_uint64, [_P]),
    "mhx_bucket_histogram": (C.c_int, [_P, C.c_int, C.c_uint32, C.c_uint32, _P]),
    "mhx_set_bucket_filter": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, C.c_int]),
    "mhx_stage_pass_bytes": (C.c_uint64, [_P, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64]),
    "mhx_stage_once_bytes": (C.c_uint64, [_P, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64]),
    "mhx_s2_from_count_bytes": (C.c_uint64, [_P, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint64]),
    "mhx_alloc_stats": (None, [_P, _P, _P, _P]),
    "mhx_alloc_peak": (None, [_P, _P, C.c_int]),
    "mhx_comm_init_hosted": (_P, [_P, C.c_int, C.c_int, _P]),
    "mhx_reset": (C.c_int, [_P]),
    "mhx_last_s1_plan": (C.c_char_p, [_P]),
    "mhx_s1_self_planned": (C.c_int, [_P, C.c_uint32, C.c_uint32, C.c_int]),
    "mhx_s1_left_items": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "mhx_count_self_planned": (C.c_int, [_P, C.c_uint32, C.c_uint32]),
    "mhx_profile_enable": (C.c_int, [_P, C.c_int]),
    "mhx_profile_reset": (C.c_int, [_P]),
    "mhx_profile_get": (C.c_int, [_P, C.POINTER(KernelStat), C.c_int]),
}

_lib = None


def load():
    """Load libmhx.so (no compute).  Raises MhxError if the HIP extension was not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MhxError("%s is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback)" % LIB_PATH)
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def local_insert_size(rec, read_len, lib_begin, lib_end, max_read_len, paired):
    """EstimateInsertSize + LocalRange of one library on the records of Engine.local_map (include/mhx.h: mhx_local_insert_size);
    host code only, needs no GPU.  rec: LOCAL_RECORD_DTYPE [n_reads], read_len: [n_reads].  -> (mean, sd, local_range)"""
    L = load()
    rec = np.ascontiguousarray(rec, dtype=LOCAL_RECORD_DTYPE)
    read_len = np.ascontiguousarray(read_len, dtype=np.uint32)
    assert lib_end <= rec.size and lib_end <= read_len.size
    mean, sd, rng = C.c_double(0), C.c_double(0), C.c_int32(0)
    if L.mhx_local_insert_size(_ptr(rec), _ptr(read_len), int(lib_begin), int(lib_end), int(max_read_len), int(bool(paired)), C.byref(mean),
                               C.byref(sd), C.byref(rng)) != 0:
        raise MhxError(L.mhx_last_error().decode())
    return mean.value, sd.value, int(rng.value)


def infer_min_depth(hist):
    """The fixed point of sdbg_pruning::InferMinDepth on a multiplicity histogram (include/mhx.h: mhx_infer_min_depth); host code
    only, needs no GPU.  hist: uint64[65536].  -> (min_depth, converged); an all-zero histogram raises ("no valid edge")."""
    L = load()
    hist = np.ascontiguousarray(hist, dtype=np.uint64)
    assert hist.shape == (MAX_MUL + 1,)
    d, conv = C.c_double(0), C.c_int(0)
    if L.mhx_infer_min_depth(_ptr(hist), C.byref(d), C.byref(conv)) != 0:
        raise MhxError(L.mhx_last_error().decode())
    return d.value, bool(conv.value)


class Engine:
    """One GPU, one HIP stream: mirrors the reference's engine objects (KmerCounter, Read2SdbgS1/S2,
    SeqToSdbg — reference src/sorting/*.h) on top of the C ABI."""

    def __init__(self, device=0):
        self.lib = load()
        self.h = self.lib.mhx_create(device)
        if not self.h:
            raise MhxError(self.lib.mhx_last_error().decode())

    def close(self):
        if self.h:
            self.lib.mhx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MhxError(self.lib.mhx_last_error().decode())

    # ---- inputs
    def load_sequences(self, packed, n_seqs, fixed_len=0, start_pos=None):
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        if start_pos is not None:
            start_pos = np.ascontiguousarray(start_pos, dtype=np.uint64)
        self._keep = (packed, start_pos)
        self._chk(self.lib.mhx_load_sequences(self.h, _ptr(packed), packed.size, n_seqs, fixed_len, _ptr(start_pos)))

    def load_bin_records(self, records, n_seqs, reverse=True):
        records = np.ascontiguousarray(records, dtype=np.uint32)
        self._chk(self.lib.mhx_load_bin_records(self.h, _ptr(records), records.size, n_seqs, int(reverse)))

    def append_sequences(self, packed, n_seqs, fixed_len=0, start_pos=None, mult=None):
        packed = np.ascontiguousarray(packed, dtype=np.uint32)
        if start_pos is not None:
            start_pos = np.ascontiguousarray(start_pos, dtype=np.uint64)
        if mult is not None:
            mult = np.ascontiguousarray(mult, dtype=np.uint16)
        self._chk(self.lib.mhx_append_sequences(self.h, _ptr(packed), packed.size, n_seqs, fixed_len, _ptr(start_pos), _ptr(mult)))

    def load_multiplicity(self, mult):
        mult = np.ascontiguousarray(mult, dtype=np.uint16)
        self._chk(self.lib.mhx_load_multiplicity(self.h, _ptr(mult), mult.size))

    def set_is_solid(self, bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint64)
        self._chk(self.lib.mhx_set_is_solid(self.h, _ptr(bits), bits.size))

    @property
    def n_seqs(self):
        return self.lib.mhx_num_sequences(self.h)

    @property
    def n_bases(self):
        return self.lib.mhx_num_bases(self.h)

    # ---- engines
    def count(self, k, m):
        r = CountResult()
        self._chk(self.lib.mhx_count(self.h, k, m, C.byref(r)))
        return r

    def read2sdbg_s1(self, k, m, want_mercy=False):
        """want_mercy: False/0 none, True/1 stable tie order, 2 reference-exact (kmsort) tie order."""
        r = S1Result()
        self._chk(self.lib.mhx_read2sdbg_s1(self.h, k, m, int(want_mercy), C.byref(r)))
        return r

    def read2sdbg_add_mercy(self, k):
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_read2sdbg_add_mercy(self.h, k, C.byref(n)))
        return n.value

    def read2sdbg_s2(self, k, m):
        r = SdbgResult()
        self._chk(self.lib.mhx_read2sdbg_s2(self.h, k, m, C.byref(r)))
        return r

    def seq2sdbg(self, k):
        r = SdbgResult()
        self._chk(self.lib.mhx_seq2sdbg(self.h, k, C.byref(r)))
        return r

    def gen_mercy_edges(self, k, cand_packed, n_cand, cand_start):
        cand_packed = np.ascontiguousarray(cand_packed, dtype=np.uint32)
        cand_start = np.ascontiguousarray(cand_start, dtype=np.uint64)
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_gen_mercy_edges(self.h, k, _ptr(cand_packed), cand_packed.size, n_cand, _ptr(cand_start),
                                               C.byref(n)))
        return n.value

    def sort_records(self, items, key_words):
        """items: uint32 [n, w]; sorted in place by the first key_words words."""
        assert items.dtype == np.uint32 and items.flags.c_contiguous and items.ndim == 2
        self._chk(self.lib.mhx_sort_records(self.h, _ptr(items), items.shape[0], key_words, items.shape[1] - key_words))
        return items

    # ---- multi-GPU phases, one call each (the C++ drivers of comm.hip compose them: lib.Comm)
    def set_partition(self, my_part, n_parts, bucket_begin):
        bb = np.ascontiguousarray(bucket_begin, dtype=np.uint32)
        self._chk(self.lib.mhx_set_partition(self.h, my_part, n_parts, _ptr(bb)))
        self.n_parts = n_parts

    def set_global_layout(self, pos_base, global_bases):
        self._chk(self.lib.mhx_set_global_layout(self.h, pos_base, global_bases))

    def dist_extract(self, stage, k, m):
        """-> (device pointer, n_items, item_bytes, counts per owner)"""
        out = DistItems()
        counts = np.zeros(self.n_parts, dtype=np.uint64)
        self._chk(self.lib.mhx_dist_extract(self.h, stage, k, m, C.byref(out), _ptr(counts)))
        return out.d_items, out.n_items, out.item_bytes, counts

    def dist_recv_buffer(self, n_items, item_bytes):
        p = self.lib.mhx_dist_recv_buffer(self.h, n_items, item_bytes)
        if not p:
            raise MhxError(self.lib.mhx_last_error().decode())
        return p

    def dist_process_s1(self, k, m, n_items, want_mercy=0):
        r = S1Result()
        self._chk(self.lib.mhx_dist_process_s1(self.h, k, m, int(want_mercy), n_items, C.byref(r)))
        return r

    def dist_process_count(self, k, m, n_items):
        r = CountResult()
        self._chk(self.lib.mhx_dist_process_count(self.h, k, m, n_items, C.byref(r)))
        return r

    def dist_process_seq2sdbg(self, k, n_items):
        r = SdbgResult()
        self._chk(self.lib.mhx_dist_process_seq2sdbg(self.h, k, n_items, C.byref(r)))
        return r

    def dist_route_records(self, which, stride_bases):
        """-> (device pointer, n_records, 8, counts per read-owning rank)"""
        out = DistItems()
        counts = np.zeros(self.n_parts, dtype=np.uint64)
        self._chk(self.lib.mhx_dist_route_records(self.h, which, stride_bases, C.byref(out), _ptr(counts)))
        return out.d_items, out.n_items, out.item_bytes, counts

    def dist_apply_routed(self, which, n_records):
        self._chk(self.lib.mhx_dist_apply_routed(self.h, which, n_records))

    def dist_process_s2(self, k, n_items):
        r = SdbgResult()
        self._chk(self.lib.mhx_dist_process_s2(self.h, k, n_items, C.byref(r)))
        return r

    def device_pointer(self, which):
        return self.lib.mhx_device_pointer(self.h, which)

    def adopt_is_solid_slice(self, ptr, n_words):
        self._chk(self.lib.mhx_adopt_is_solid_slice(self.h, ptr, n_words))

    # ---- memory-bounded passes (see megahit_amd/passes.py)
    def bucket_histogram(self, stage, k, m):
        h = np.zeros(NUM_BUCKETS, dtype=np.uint64)
        self._chk(self.lib.mhx_bucket_histogram(self.h, stage, k, m, _ptr(h)))
        return h

    def set_bucket_filter(self, keep, expected_items=0, batch_bytes=0, accumulate=False):
        if keep is None:
            self._chk(self.lib.mhx_set_bucket_filter(self.h, None, 0, batch_bytes, int(accumulate)))
            return
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        assert keep.size == NUM_BUCKETS
        self._chk(self.lib.mhx_set_bucket_filter(self.h, _ptr(keep), int(expected_items), int(batch_bytes), int(accumulate)))

    # ---- outputs
    def fetch(self, which, dtype):
        nbytes = self.lib.mhx_buffer_bytes(self.h, which)
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype=dtype)
        if nbytes:
            self._chk(self.lib.mhx_fetch(self.h, which, _ptr(out), 0, nbytes))
        return out

    def fetch_range(self, which, dtype, offset, count):
        """`count` elements of `dtype` from element `offset` of a result buffer (the offset argument of mhx_fetch): a look at a part of
        a buffer too large to bring over whole; a range beyond the buffer raises"""
        size = np.dtype(dtype).itemsize
        out = np.empty(int(count), dtype=dtype)
        if count:
            self._chk(self.lib.mhx_fetch(self.h, which, _ptr(out), int(offset) * size, int(count) * size))
        return out

    def synchronize(self):
        self._chk(self.lib.mhx_synchronize(self.h))

    def trim(self):
        self._chk(self.lib.mhx_trim(self.h))

    def alloc_peak(self, reset=False):
        """-> (device bytes the library's buffers of this process hold now, their high-water mark); reset: the mark restarts
        at the bytes held now (mhx_alloc_peak; process-wide, not per handle)"""
        held, peak = C.c_uint64(0), C.c_uint64(0)
        self.lib.mhx_alloc_peak(C.byref(held), C.byref(peak), int(reset))
        return int(held.value), int(peak.value)

    def stage_pass_bytes(self, stage, k, m, n_items):
        """device bytes the memory plan assumes for a pass of `stage` over n_items kept items (mhx_stage_pass_bytes)"""
        return int(self.lib.mhx_stage_pass_bytes(self.h, stage, k, m, int(n_items)))

    def stage_once_bytes(self, stage, k, m, n_items):
        """device bytes the memory plan assumes for one unfiltered run of `stage` where that has a leaner route; 0: none
        (mhx_stage_once_bytes)"""
        return int(self.lib.mhx_stage_once_bytes(self.h, stage, k, m, int(n_items)))

    def s2_from_count_bytes(self, k, m, est_items, pass_records=0):
        """device bytes stage 2 from a count of the (k+1)-mers holds with its count in passes of at most pass_records records (0: everything
        at once); 0: the route does not apply (mhx_s2_from_count_bytes)"""
        return int(self.lib.mhx_s2_from_count_bytes(self.h, k, m, int(est_items), int(pass_records)))

    def fastx_to_records(self, text1, text2=None):
        """FASTA/FASTQ text -> read-library records on the GPU; returns (FastxResult, uint32 records or None)."""
        r = FastxResult()
        self._chk(self.lib.mhx_fastx_to_records(self.h, text1, len(text1), text2, len(text2) if text2 is not None else 0, C.byref(r)))
        return r, (self.fetch(BUF_LIB_RECORDS, np.uint32) if r.status == 0 else None)

    def bgzf_inflate(self, gz):
        """A BGZF file's bytes inflated on the GPU, one block per wavefront, every block checked against its CRC32 and ISIZE
        (include/mhx.h: mhx_bgzf_inflate); returns (BgzfResult, the text as bytes, or None when status != 0)."""
        r = BgzfResult()
        self._chk(self.lib.mhx_bgzf_inflate(self.h, gz, len(gz), C.byref(r)))
        return r, (self.fetch(BUF_FASTX_TEXT, np.uint8).tobytes() if r.status == 0 else None)

    def fastx_bgzf_to_records(self, gz1, gz2=None):
        """fastx_to_records on the texts of one or two BGZF files, inflated on the GPU and parsed where they lie; status 2: a file was
        not inflated there.  Returns (FastxResult, uint32 records or None)."""
        r = FastxResult()
        self._chk(self.lib.mhx_fastx_bgzf_to_records(self.h, gz1, len(gz1), gz2, len(gz2) if gz2 is not None else 0, C.byref(r)))
        return r, (self.fetch(BUF_LIB_RECORDS, np.uint32) if r.status == 0 else None)

    # ---- `local`, first half (include/mhx.h: mhx_local_*)
    def local_index(self, contig_packed, n_contigs, contig_start, seed_kmer=31, sparsity=8):
        """the seed index over the (kept, forward) contigs; returns the number of distinct keys"""
        contig_packed = np.ascontiguousarray(contig_packed, dtype=np.uint32)
        contig_start = np.ascontiguousarray(contig_start, dtype=np.uint64)
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_local_index(self.h, _ptr(contig_packed), contig_packed.size, int(n_contigs), _ptr(contig_start), int(seed_kmer),
                                           int(sparsity), C.byref(n)))
        return int(n.value)

    def local_map(self, min_mapping_len=75, similarity=0.8):
        """TryMap of every loaded (forward) read into BUF_LOCAL_REC; returns the number of valid records"""
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_local_map(self.h, int(min_mapping_len), float(similarity), C.byref(n)))
        return int(n.value)

    def local_records(self):
        return self.fetch(BUF_LOCAL_REC, np.uint8).view(LOCAL_RECORD_DTYPE)

    def local_collect(self, libs):
        """libs: [(begin, end, paired, local_range)] -> (aligned per library, added per library, items uint64, offsets uint64)"""
        b = np.array([l[0] for l in libs], dtype=np.uint64)
        e = np.array([l[1] for l in libs], dtype=np.uint64)
        p = np.array([int(bool(l[2])) for l in libs], dtype=np.int32)
        r = np.array([l[3] for l in libs], dtype=np.int32)
        nm, na = np.zeros(len(libs), dtype=np.uint64), np.zeros(len(libs), dtype=np.uint64)
        self._chk(self.lib.mhx_local_collect(self.h, len(libs), _ptr(b), _ptr(e), _ptr(p), _ptr(r), _ptr(nm), _ptr(na)))
        return nm, na, self.fetch(BUF_LOCAL_ITEMS, np.uint64), self.fetch(BUF_LOCAL_OFFSETS, np.uint64)

    def sdbg_build_index(self, k):
        """W/last/tip/mul arrays + rank/select tables on the device (include/mhx.h: mhx_sdbg_build_index)."""
        info = SdbgIndexInfo()
        self._chk(self.lib.mhx_sdbg_build_index(self.h, k, C.byref(info)))
        return info

    def sdbg_remove_tips(self, info, max_tip_len):
        """sdbg_pruning::RemoveTips on the device-resident graph; returns the number of tips removed."""
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_sdbg_remove_tips(self.h, C.byref(info), int(max_tip_len), C.byref(n)))
        return int(n.value)

    def sdbg_mul_histogram(self, info):
        """Histogram of EdgeMultiplicity over the edges that are valid now (include/mhx.h: mhx_sdbg_mul_histogram);
        returns (hist uint64[65536] fetched from BUF_SDBG_MUL_HIST, n_valid)."""
        self._chk(self.lib.mhx_sdbg_mul_histogram(self.h, C.byref(info), None))  # (no n_valid: the bins come over once, in the fetch)
        hist = self.fetch(BUF_SDBG_MUL_HIST, np.uint64)
        return hist, int(hist.sum())

    def sdbg_infer_min_depth(self, info):
        """sdbg_pruning::InferMinDepth on the device-resident graph as it is now (include/mhx.h: mhx_sdbg_infer_min_depth);
        returns (min_depth, converged)."""
        d, conv = C.c_double(0), C.c_int(0)
        self._chk(self.lib.mhx_sdbg_infer_min_depth(self.h, C.byref(info), C.byref(d), C.byref(conv)))
        return d.value, bool(conv.value)

    def sdbg_unitigs(self, info):
        """The unitig graph of the device-resident graph (include/mhx.h: mhx_sdbg_unitigs); returns a UnitigResult.  The
        vertices (UNITIG_VERTEX_DTYPE), the contig text and its offsets stay on the device: BUF_UNITIG_*."""
        r = UnitigResult()
        self._chk(self.lib.mhx_sdbg_unitigs(self.h, C.byref(info), C.byref(r)))
        return r

    def unitig_disconnect_weak_links(self, info, ratio):
        """DisconnectWeakLinks + Refresh on the unitig graph of the last sdbg_unitigs call (include/mhx.h:
        mhx_unitig_disconnect_weak_links); returns the number of (vertex, strand) flags set."""
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_unitig_disconnect_weak_links(self.h, C.byref(info), float(ratio), C.byref(n)))
        return int(n.value)

    def unitig_remove_tips(self, info, max_tip_len):
        """RemoveTips on the unitig graph, a Refresh after every threshold (include/mhx.h: mhx_unitig_remove_tips);
        returns the number of tips removed."""
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_unitig_remove_tips(self.h, C.byref(info), int(max_tip_len), C.byref(n)))
        return int(n.value)

    def unitig_remove_local_low_depth(self, info, min_depth, max_len, local_width=1000, local_ratio=0.2, mark_changed=False):
        """One RemoveLocalLowDepth pass, with its Refresh when something was deleted (include/mhx.h:
        mhx_unitig_remove_local_low_depth); returns (vertices deleted, is_changed).  mark_changed: survivors of merges get
        UNITIG_CHANGED."""
        n, chg = C.c_uint64(0), C.c_int(0)
        self._chk(self.lib.mhx_unitig_remove_local_low_depth(self.h, C.byref(info), float(min_depth), int(max_len), int(local_width),
                                                             float(local_ratio), int(bool(mark_changed)), C.byref(n), C.byref(chg)))
        return n.value, bool(chg.value)

    def unitig_iterate_local_low_depth(self, info, min_depth, max_len, local_width=1000, local_ratio=0.2, mark_changed=False):
        """IterateLocalLowDepth: passes at min_depth, 1.1 * min_depth, ... until one changes nothing (include/mhx.h:
        mhx_unitig_iterate_local_low_depth); returns the vertices deleted in all."""
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_unitig_iterate_local_low_depth(self.h, C.byref(info), float(min_depth), int(max_len), int(local_width),
                                                              float(local_ratio), int(bool(mark_changed)), C.byref(n)))
        return n.value

    def unitig_finish(self, info):
        """Flags, contig text and offsets of the cleaned vertex table (include/mhx.h: mhx_unitig_finish); returns a
        UnitigResult.  unitig_contigs() then returns the cleaned graph."""
        r = UnitigResult()
        self._chk(self.lib.mhx_unitig_finish(self.h, C.byref(info), C.byref(r)))
        return r

    def unitig_pop_bubbles(self, info, max_len, similarity=0.0, careful_threshold=-1.0, mark_changed=False):
        """One PopBubbles pass with its Refresh (include/mhx.h: mhx_unitig_pop_bubbles); returns (vertices deleted, careful
        records).  similarity <= 0: the naive remover (max_len = k + 2); > 0: the complex one (max_len = lround(merge_len * k /
        similarity)).  careful_threshold >= 0 leaves the --careful_bubble records for unitig_bubble_records()."""
        n, r = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.mhx_unitig_pop_bubbles(self.h, C.byref(info), int(max_len), float(similarity), float(careful_threshold),
                                                  int(bool(mark_changed)), C.byref(n), C.byref(r)))
        return int(n.value), int(r.value)

    def unitig_bubble_records(self):
        """-> [(text, average depth, vertex)] of the last unitig_pop_bubbles call, in the reference's -t 1 order."""
        rec = self.fetch(BUF_UNITIG_BUBBLE_REC, np.uint8).view(BUBBLE_RECORD_DTYPE)
        seq = self.fetch(BUF_UNITIG_BUBBLE_SEQ, np.uint8).tobytes().decode()
        return [(seq[int(r["offset"]):int(r["offset"]) + int(r["length"])], float(r["avg_depth"]), int(r["vertex"])) for r in rec]

    def unitig_bubble_stats(self):
        """-> dict(candidates, passed, failed, finishes) of the last unitig_pop_bubbles call (mhx_unitig_bubble_stats)."""
        out = (C.c_uint64 * 4)()
        self._chk(self.lib.mhx_unitig_bubble_stats(self.h, out))
        return dict(zip(("candidates", "passed", "failed", "finishes"), (int(x) for x in out)))

    def unitig_remove_low_depth(self, info, min_depth):
        """RemoveLowDepth + Refresh: every vertex with average depth < min_depth goes (include/mhx.h:
        mhx_unitig_remove_low_depth); returns the vertices deleted."""
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_unitig_remove_low_depth(self.h, C.byref(info), float(min_depth), C.byref(n)))
        return int(n.value)

    def unitig_similarity(self, a, b, similarity):
        """GetSimilarity of two strings by the device kernel of the complex bubble remover (include/mhx.h:
        mhx_unitig_similarity); returns the double.  Beyond SIM_MAX_LEN / SIM_MAX_INDEL it raises."""
        a, b = (x.encode() if isinstance(x, str) else bytes(x) for x in (a, b))
        out = C.c_double(0)
        self._chk(self.lib.mhx_unitig_similarity(self.h, a, len(a), b, len(b), float(similarity), C.byref(out)))
        return out.value

    def unitig_contigs(self):
        """-> (vertices as a UNITIG_VERTEX_DTYPE array, list of contig strings) of the last sdbg_unitigs / unitig_finish call."""
        v = self.fetch(BUF_UNITIG_VERTICES, np.uint8).view(UNITIG_VERTEX_DTYPE)
        seq = self.fetch(BUF_UNITIG_SEQ, np.uint8).tobytes().decode()
        off = self.fetch(BUF_UNITIG_OFFSET, np.uint64)
        return v, [seq[off[i]:off[i + 1]] for i in range(v.size)]

    def sdbg_load_bytes(self, data, offset, items, tips, large):
        data = np.ascontiguousarray(data, dtype=np.uint8)
        tabs = [np.ascontiguousarray(t, dtype=np.uint64) for t in (offset, items, tips, large)]
        self._chk(self.lib.mhx_sdbg_load_bytes(self.h, _ptr(data), data.size, *[_ptr(t) for t in tabs]))

    def set_option(self, name, value):
        """Tuning / diagnostic knob of this handle (include/mhx.h: mhx_set_option)."""
        self._chk(self.lib.mhx_set_option(self.h, name.encode(), int(value)))

    def s1_self_planned(self, k, min_count, want_mercy=False):
        """stage 1 would run on super-k-mer records and cut the job into passes by itself (mhx_s1_self_planned)"""
        return bool(self.lib.mhx_s1_self_planned(self.h, k, min_count, int(want_mercy)))

    def count_self_planned(self, k, min_count):
        """count would run on super-k-mer records and cut the job into passes by itself (mhx_count_self_planned)"""
        return bool(self.lib.mhx_count_self_planned(self.h, k, min_count))

    def s1_left_items(self, k, min_count):
        """the handle holds the aggregated stage-2 items stage 1 left for (k, min_count) (mhx_s1_left_items)"""
        return bool(self.lib.mhx_s1_left_items(self.h, k, min_count))

    def last_s1_plan(self):
        """what the last stage 1 of this handle ran as (mhx_last_s1_plan)"""
        return (self.lib.mhx_last_s1_plan(self.h) or b"").decode()

    def get_option(self, name, default):
        """Effective value of a knob for this handle (include/mhx.h: mhx_get_option): explicit option, environment, tuned default."""
        return int(self.lib.mhx_get_option(self.h, name.encode(), int(default)))

    # ---- profiling
    def profile(self, on=True):
        self._chk(self.lib.mhx_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self._chk(self.lib.mhx_profile_reset(self.h))

    def profile_get(self):
        arr = (KernelStat * 128)()
        n = self.lib.mhx_profile_get(self.h, arr, 128)
        if n < 0:
            raise MhxError(self.lib.mhx_last_error().decode())
        return {arr[i].name.decode(): dict(launches=arr[i].launches, ms=arr[i].total_ms, bytes=arr[i].algo_bytes)
                for i in range(min(n, 128))}


COMM_ID_BYTES = 128


def comm_unique_id():
    """RCCL unique id (bytes) created by one rank and shipped to the others (mhx_comm_unique_id)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    if load().mhx_comm_unique_id(buf) != 0:
        raise MhxError(load().mhx_last_error().decode())
    return buf.raw


class Comm:
    """Communicator of the C++ multi-GPU drivers (include/mhx.h: mhx_comm_*).  One per rank, bound to the rank's Engine."""

    def __init__(self, engine, handle):
        self.lib, self.e, self.h = engine.lib, engine, handle

    @classmethod
    def rccl(cls, engine, unique_id, rank, n_ranks):
        h = engine.lib.mhx_comm_init_rank(engine.h, unique_id, rank, n_ranks)
        if not h:
            raise MhxError(engine.lib.mhx_last_error().decode())
        return cls(engine, h)

    @classmethod
    def hosted(cls, engine, dist, rank, n_ranks):
        """The caller's torch.distributed group (any backend that moves CPU tensors, e.g. gloo) moves the bytes through host
        memory (megahit_amd/hosted.py): rank processes that cannot share an RCCL world, e.g. several on one GPU."""
        from . import hosted as H
        t, keep = H.make_transport(dist, rank, n_ranks)
        engine.lib.mhx_comm_init_hosted.restype = C.c_void_p
        engine.lib.mhx_comm_init_hosted.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(H.HostTransport)]
        h = engine.lib.mhx_comm_init_hosted(engine.h, rank, n_ranks, C.byref(t))
        if not h:
            raise MhxError(engine.lib.mhx_last_error().decode())
        cm = cls(engine, h)
        cm._keep = (t, keep)  # the callbacks must outlive the communicator
        return cm

    @classmethod
    def local_group(cls, engines):
        """In-process group (no RCCL): the ranks are threads of this process and may share GPUs."""
        n = len(engines)
        ctxs = (C.c_void_p * n)(*[e.h for e in engines])
        out = (C.c_void_p * n)()
        if engines[0].lib.mhx_comm_local_group(n, ctxs, out) != 0:
            raise MhxError(engines[0].lib.mhx_last_error().decode())
        return [cls(e, out[i]) for i, e in enumerate(engines)]

    def close(self):
        if self.h:
            self.lib.mhx_comm_destroy(self.h)
            self.h = None

    def _chk(self, rc):
        if rc != 0:
            raise MhxError(self.lib.mhx_last_error().decode())

    def barrier(self):
        self._chk(self.lib.mhx_comm_barrier(self.h))

    def bytes_sent(self, reset=False):
        """payload bytes this rank has handed to other ranks through the item / record exchanges since the last reset"""
        return int(self.lib.mhx_comm_bytes_sent(self.h, int(reset)))

    def all_reduce(self, values, is_max=False):
        v = np.ascontiguousarray(values, dtype=np.uint64).copy()
        self._chk(self.lib.mhx_comm_all_reduce_u64(self.h, _ptr(v), v.size, int(is_max)))
        return v

    def setup(self, balance_stage=0, k=21, m=2):
        self._chk(self.lib.mhx_dist_setup(self.e.h, self.h, balance_stage, k, m))

    def read2sdbg(self, k, m, need_mercy=0):
        r1, r2, nm = S1Result(), SdbgResult(), C.c_uint64(0)
        self._chk(self.lib.mhx_dist_read2sdbg(self.e.h, self.h, k, m, int(need_mercy), C.byref(r1), C.byref(r2), C.byref(nm)))
        return r1, r2, int(nm.value)

    def count(self, k, m):
        r = CountResult()
        self._chk(self.lib.mhx_dist_count(self.e.h, self.h, k, m, C.byref(r)))
        return r

    def seq2sdbg(self, k):
        r = SdbgResult()
        self._chk(self.lib.mhx_dist_seq2sdbg(self.e.h, self.h, k, C.byref(r)))
        return r

    def gen_mercy_edges(self, k, cand_packed, n_cand, cand_start):
        """collective: every rank passes ALL candidate reads; returns the number of all mercy edges"""
        cand_packed = np.ascontiguousarray(cand_packed, dtype=np.uint32)
        cand_start = np.ascontiguousarray(cand_start, dtype=np.uint64)
        n = C.c_uint64(0)
        self._chk(self.lib.mhx_dist_gen_mercy_edges(self.e.h, self.h, k, _ptr(cand_packed), cand_packed.size, n_cand, _ptr(cand_start), C.byref(n)))
        return n.value
