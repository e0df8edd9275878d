"""ctypes binding of include/cvtmi.h.

There is NO fallback: if libcvtmi.so is missing or a call fails, an exception is raised.  Arrays
may be numpy (host-pointer entry points) or torch CUDA tensors (``*_dev`` entry points on the
tensor's device, launched on torch's current stream so torch events/streams order them).
"""
import contextlib
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CVTMI_LIB") or os.path.join(_HERE, "lib", "libcvtmi.so")   # CVTMI_LIB: an instrumented / experimental build
_lib = None


class CvtmiError(RuntimeError):
    pass


def _torch_first():
    """One HIP runtime per process.  libcvtmi.so asks the loader for libamdhip64 / libhsa-runtime64 by SONAME; a PyTorch-ROCm wheel carries
    its own copies under torch/lib.  Whoever loads first decides which copy the SONAME resolves to, and a process that ends up with the
    system libamdhip64 over the wheel's HSA runtime (library first, torch second) sees "no ROCm-capable device".  So where torch is
    installed it is imported before the library; without torch (a C / ctypes host) the system ROCm is the only runtime and nothing is done."""
    import sys
    if "torch" in sys.modules:
        return
    import importlib.util
    if importlib.util.find_spec("torch") is not None:
        import torch  # noqa: F401


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise CvtmiError("libcvtmi.so not built (%s): run `python -c 'import __graft_entry__ as g; g.build()'` "
                             "or `make -C cvt_amd/csrc`" % LIB_PATH)
        _torch_first()
        _lib = C.CDLL(LIB_PATH)
        _lib.cvtmi_last_error.restype = C.c_char_p
    return _lib


def lib():
    return load_library()


ESPACE = -7   # CVTMI_ESPACE: the result does not fit the caller's arrays


def _check(rc):
    if rc != 0:
        err = CvtmiError("cvtmi error %d: %s" % (rc, lib().cvtmi_last_error().decode(errors="replace")))
        err.code = rc
        raise err


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def _ptr(a):
    if a is None:
        return C.c_void_p(0)
    if _is_torch(a):
        assert a.is_contiguous()
        return C.c_void_p(a.data_ptr())
    assert a.flags["C_CONTIGUOUS"]
    return C.c_void_p(a.ctypes.data)


def _stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


class _LaunchRecord(C.Structure):
    _fields_ = [("name", C.c_char * 64), ("grid", C.c_int64 * 3), ("block", C.c_int64), ("lds", C.c_int64)]


@contextlib.contextmanager
def launch_log():
    """``with launch_log() as log:`` -- the kernels the calling thread launches inside the block (cvtmi_debug_launch_log_*): `log` is a
    list that is filled when the block ends with one (name, (grid x, y, z), block x, dynamic LDS bytes) per launch, in launch order.
    Blocks nest (an inner block's launches are in the outer list too); other threads' launches are never seen."""
    L = lib()
    for f in (L.cvtmi_debug_launch_log_begin, L.cvtmi_debug_launch_log_end, L.cvtmi_debug_launch_log_read):
        f.restype = C.c_int64
    L.cvtmi_debug_launch_log_read.argtypes = [C.c_int64, C.c_int64, C.POINTER(_LaunchRecord)]
    log = []
    mark = L.cvtmi_debug_launch_log_begin()
    try:
        yield log
    finally:
        total = L.cvtmi_debug_launch_log_end()
        if total < 0:
            _check(int(total))
        count = max(0, total - mark)
        recs = (_LaunchRecord * max(1, count))()
        L.cvtmi_debug_launch_log_read(mark, count, recs)
        log.extend((r.name.decode(), tuple(r.grid), int(r.block), int(r.lds)) for r in recs[:count])


def device_count():
    n = C.c_int(0)
    _check(lib().cvtmi_device_count(C.byref(n)))
    return n.value


class OpqIndex:
    """cvtmi_opq_t: OPQ model (coarse, sub-codebooks, rotation) + HBM-resident code index."""

    def __init__(self, coarse, books, perm=None, R=None):
        coarse = _np(coarse, np.float32); books = _np(books, np.float32)
        self.coarseK, self.D = coarse.shape
        self.M, self.K, step = books.shape
        assert self.M * step == self.D
        perm_a = None if perm is None else _np(perm, np.int32)
        R_a = None if R is None else _np(R, np.float32)
        self.h = C.c_void_p(0)
        _check(lib().cvtmi_opq_create(C.c_int(self.D), C.c_int(self.coarseK), C.c_int(self.M), C.c_int(self.K),
                                      _ptr(coarse), _ptr(books), _ptr(R_a), _ptr(perm_a), C.byref(self.h)))

    def close(self):
        if self.h and self.h.value:
            lib().cvtmi_opq_destroy(self.h)
            self.h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- rotate ----
    def rotate(self, x):
        if _is_torch(x):
            import torch
            y = torch.empty_like(x)
            _check(lib().cvtmi_opq_rotate_dev(self.h, _ptr(x), C.c_int64(x.shape[0]), _ptr(y), _stream()))
            return y
        x = _np(x, np.float32)
        y = np.empty_like(x)
        _check(lib().cvtmi_opq_rotate(self.h, _ptr(x), C.c_int64(x.shape[0]), _ptr(y)))
        return y

    # ---- encode ----
    def encode(self, x_rot):
        n = x_rot.shape[0]
        if _is_torch(x_rot):
            import torch
            lists = torch.empty(n, dtype=torch.int32, device=x_rot.device)
            codes = torch.empty((n, self.M), dtype=torch.uint8, device=x_rot.device)
            _check(lib().cvtmi_opq_encode_dev(self.h, _ptr(x_rot), C.c_int64(n), _ptr(lists), _ptr(codes), _stream()))
            return lists, codes
        x_rot = _np(x_rot, np.float32)
        lists = np.empty(n, dtype=np.int32)
        codes = np.empty((n, self.M), dtype=np.uint8)
        _check(lib().cvtmi_opq_encode(self.h, _ptr(x_rot), C.c_int64(n), _ptr(lists), _ptr(codes)))
        return lists, codes

    def rotate_encode(self, x):
        """rotate + encode of RAW rows (cvtmi_opq_rotate_encode): (list ids, codes)"""
        n = x.shape[0]
        if _is_torch(x):
            import torch
            lists = torch.empty(n, dtype=torch.int32, device=x.device)
            codes = torch.empty((n, self.M), dtype=torch.uint8, device=x.device)
            _check(lib().cvtmi_opq_rotate_encode_dev(self.h, _ptr(x), C.c_int64(n), _ptr(lists), _ptr(codes), _stream()))
            return lists, codes
        x = _np(x, np.float32)
        lists = np.empty(n, dtype=np.int32)
        codes = np.empty((n, self.M), dtype=np.uint8)
        _check(lib().cvtmi_opq_rotate_encode(self.h, _ptr(x), C.c_int64(n), _ptr(lists), _ptr(codes)))
        return lists, codes

    # ---- index ----
    def add_codes(self, codes, list_id=None, video_id=None):
        n = codes.shape[0]
        if _is_torch(codes):
            _check(lib().cvtmi_opq_add_codes_dev(self.h, _ptr(codes), _ptr(list_id), _ptr(video_id), C.c_int64(n),
                                                 _stream()))
            return
        codes = _np(codes, np.uint8)
        l = None if list_id is None else _np(list_id, np.int32)
        v = None if video_id is None else _np(video_id, np.int32)
        _check(lib().cvtmi_opq_add_codes(self.h, _ptr(codes), _ptr(l), _ptr(v), C.c_int64(n)))

    def reserve(self, n):
        _check(lib().cvtmi_opq_reserve(self.h, C.c_int64(n)))

    def reset(self):
        _check(lib().cvtmi_opq_reset(self.h))

    @property
    def ntotal(self):
        n = C.c_int64(0)
        _check(lib().cvtmi_opq_ntotal(self.h, C.byref(n)))
        return n.value

    def set_id_base(self, base):
        _check(lib().cvtmi_opq_set_id_base(self.h, C.c_int64(base)))

    def get_entries(self):
        n = self.ntotal
        off = np.empty(self.coarseK + 1, dtype=np.int64)
        vid = np.empty(n, dtype=np.int32)
        codes = np.empty((n, self.M), dtype=np.uint8)
        _check(lib().cvtmi_opq_get_entries(self.h, _ptr(off), _ptr(vid), _ptr(codes)))
        tot = int(off[-1])
        return off, vid[:tot], codes[:tot]

    # ---- removal ----
    def _remove(self, fn, ids, dt, extra, want_remap):
        n0 = self.ntotal
        removed = C.c_int64(0)
        if _is_torch(ids):
            import torch
            assert ids.dtype == getattr(torch, dt) and ids.is_cuda
            remap = torch.empty(n0, dtype=torch.int64, device=ids.device) if want_remap else None
            _check(getattr(lib(), fn + "_dev")(self.h, _ptr(ids), C.c_int64(ids.shape[0]), *extra, C.byref(removed), _ptr(remap), _stream()))
        else:
            ids = _np(ids, dt).reshape(-1)
            remap = np.empty(n0, dtype=np.int64) if want_remap else None
            _check(getattr(lib(), fn)(self.h, _ptr(ids), C.c_int64(ids.shape[0]), *extra, C.byref(removed), _ptr(remap)))
        return (removed.value, remap) if want_remap else removed.value

    def remove_videos(self, video_ids, renumber=False, want_remap=False):
        """Drop every entry whose video id is in `video_ids` (cvtmi_opq_remove_videos; int32, numpy or a torch device tensor).  The kept
        entries close up in insertion order; renumber=True lowers every kept video id by the number of distinct removed ids below
        it.  Returns the number of entries dropped, with want_remap (dropped, remap): remap[i] = new insertion index of old entry
        i, or -1."""
        return self._remove("cvtmi_opq_remove_videos", video_ids, "int32", (C.c_int(1 if renumber else 0),), want_remap)

    def remove_ids(self, ids, want_remap=False):
        """Drop every entry whose id (id_base + insertion index, what the searches report) is in `ids` (cvtmi_opq_remove_ids; int64,
        numpy or a torch device tensor).  Returns like remove_videos."""
        return self._remove("cvtmi_opq_remove_ids", ids, "int64", (), want_remap)

    # ---- query ----
    def lut(self, q_rot, list_id=None):
        nq = q_rot.shape[0]
        if _is_torch(q_rot):
            import torch
            out = torch.empty((nq, self.M, self.K), dtype=torch.float32, device=q_rot.device)
            _check(lib().cvtmi_opq_lut_dev(self.h, _ptr(q_rot), C.c_int64(nq), _ptr(list_id), _ptr(out), _stream()))
            return out
        q_rot = _np(q_rot, np.float32)
        l = None if list_id is None else _np(list_id, np.int32)
        out = np.empty((nq, self.M, self.K), dtype=np.float32)
        _check(lib().cvtmi_opq_lut(self.h, _ptr(q_rot), C.c_int64(nq), _ptr(l), _ptr(out)))
        return out

    def search(self, q, k, rotate=True, out=None):
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            if out is None:
                d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
                i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            else:
                d, i = out
            _check(lib().cvtmi_opq_search_dev(self.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(k),
                                              _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, np.float32)
        if out is None:
            d = np.empty((nq, k), dtype=np.float32); i = np.empty((nq, k), dtype=np.int64)
        else:   # the caller's own (already touched) arrays: freshly allocated ones cost a page fault per 4 KB written
            d, i = out
            assert d.dtype == np.float32 and i.dtype == np.int64 and d.shape == (nq, k) and i.shape == (nq, k)
            assert d.flags.c_contiguous and i.flags.c_contiguous
        _check(lib().cvtmi_opq_search(self.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(k),
                                      _ptr(d), _ptr(i)))
        return d, i

    def search_sharded(self, comm, q, k, rotate=True):
        """Row-sharded search: this handle holds the rank's row block; one all-gather + merge inside the library.
        Device tensors: nothing synchronises, so another rank's failure cannot be known when this returns -- its results are
        voided on the device (+inf / -1) and the error is raised by the next call on `comm`, by comm.status() after a
        synchronise, or at the latest by comm.close()."""
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            comm.check(lib().cvtmi_opq_search_sharded_dev(self.h, comm.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0),
                                                      C.c_int(k), _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, np.float32)
        d = np.empty((nq, k), dtype=np.float32); i = np.empty((nq, k), dtype=np.int64)
        comm.check(lib().cvtmi_opq_search_sharded(self.h, comm.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(k),
                                              _ptr(d), _ptr(i)))
        return d, i

    def query_video(self, q, nprobe, img_num, rotate=True):
        if _is_torch(q):
            import torch
            ms = torch.empty((q.shape[0], img_num), dtype=torch.float32, device=q.device)
            _check(lib().cvtmi_opq_query_video_dev(self.h, _ptr(q), C.c_int64(q.shape[0]), C.c_int(1 if rotate else 0),
                                                   C.c_int(nprobe), C.c_int(img_num), _ptr(ms), _stream()))
            return ms
        q = _np(q, np.float32)
        ms = np.empty((q.shape[0], img_num), dtype=np.float32)
        _check(lib().cvtmi_opq_query_video(self.h, _ptr(q), C.c_int64(q.shape[0]), C.c_int(1 if rotate else 0),
                                           C.c_int(nprobe), C.c_int(img_num), _ptr(ms)))
        return ms

    def rank_videos(self, q, seg_off, nprobe, img_num, k, rotate=True, want_total=False):
        """The reference's whole query for several query videos at once (cvtmi_opq_rank_videos): segment s is frames seg_off[s] ..
        seg_off[s + 1] - 1 of q; per segment the rows of query_video are added up in frame order and the k smallest (total, video)
        pairs are returned: (score [nseg][k] float32, video [nseg][k] int64), padded with (+inf, -1), and with want_total the totals
        [nseg][img_num] as well.  seg_off is read on the host (a list, numpy or a CPU tensor) whatever q is."""
        seg = np.ascontiguousarray(np.asarray(seg_off.cpu() if _is_torch(seg_off) else seg_off), dtype=np.int64).reshape(-1)
        assert seg.shape[0] >= 1, "seg_off holds nseg + 1 offsets"
        nseg = seg.shape[0] - 1
        args = (C.c_int64(nseg), C.c_int(1 if rotate else 0), C.c_int(nprobe), C.c_int(img_num), C.c_int(k))
        if _is_torch(q):
            import torch
            s = torch.empty((nseg, k), dtype=torch.float32, device=q.device)
            v = torch.empty((nseg, k), dtype=torch.int64, device=q.device)
            t = torch.empty((nseg, img_num), dtype=torch.float32, device=q.device) if want_total else None
            _check(lib().cvtmi_opq_rank_videos_dev(self.h, _ptr(q), _ptr(seg), *args, _ptr(s), _ptr(v), _ptr(t), _stream()))
        else:
            q = _np(q, np.float32)
            s = np.empty((nseg, k), dtype=np.float32); v = np.empty((nseg, k), dtype=np.int64)
            t = np.empty((nseg, img_num), dtype=np.float32) if want_total else None
            _check(lib().cvtmi_opq_rank_videos(self.h, _ptr(q), _ptr(seg), *args, _ptr(s), _ptr(v), _ptr(t)))
        return (s, v, t) if want_total else (s, v)

    def last_rank(self):
        """chunks and scratch areas of the last rank_videos on this handle (cvtmi_opq_last_rank)"""
        o = (C.c_int64 * 4)()
        _check(lib().cvtmi_opq_last_rank(self.h, o))
        return dict(chunks=o[0], frames_per_chunk=o[1], score_bytes=o[2], total_bytes=o[3])

    def search_ivf(self, q, nprobe, k, rotate=True, out=None):
        """Row-level IVF search (cvtmi_opq_search_ivf): the k nearest entries among the nprobe nearest coarse lists of every query:
        (distances [nq][k] float32, ids [nq][k] int64), padded with (+inf, -1)."""
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            if out is None:
                d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
                i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            else:
                d, i = out
            _check(lib().cvtmi_opq_search_ivf_dev(self.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(nprobe),
                                                  C.c_int(k), _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, np.float32)
        if out is None:
            d = np.empty((nq, k), dtype=np.float32); i = np.empty((nq, k), dtype=np.int64)
        else:
            d, i = out
            assert d.dtype == np.float32 and i.dtype == np.int64 and d.shape == (nq, k) and i.shape == (nq, k)
            assert d.flags.c_contiguous and i.flags.c_contiguous
        _check(lib().cvtmi_opq_search_ivf(self.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(nprobe), C.c_int(k),
                                          _ptr(d), _ptr(i)))
        return d, i

    def search_refine(self, flat, q, k, R, nprobe=0, rotate=True):
        """ADC candidates, exact finish (cvtmi_opq_search_refine): the R best entries of search_ivf(nprobe) -- nprobe = 0: of search,
        which needs coarseK == 1 -- reranked against the FlatIndex `flat` (the same rows, fp32) with the raw queries:
        (exact distances [nq][k] float32, the flat index's labels [nq][k] int64).  The candidate lists never leave the device."""
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            _check(lib().cvtmi_opq_search_refine_dev(self.h, flat.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(nprobe),
                                                     C.c_int(k), C.c_int(R), _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, np.float32)
        d = np.empty((nq, k), dtype=np.float32); i = np.empty((nq, k), dtype=np.int64)
        _check(lib().cvtmi_opq_search_refine(self.h, flat.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(nprobe), C.c_int(k),
                                             C.c_int(R), _ptr(d), _ptr(i)))
        return d, i

    def last_ivf_plan(self):
        """grid of the last search_ivf on this handle (cvtmi_opq_last_ivf_plan)"""
        o = (C.c_int64 * 8)()
        _check(lib().cvtmi_opq_last_ivf_plan(self.h, o))
        return dict(rule=o[0], G=o[1], groups=o[2], pieces=o[3], rows_per_piece=o[4], parts=o[5], part_bytes=o[6], entry_bytes=o[7])

    def _mask_words(self, mask, dev):
        """`mask` as uint64 words (bit i & 63 of word i >> 6 = insertion index i), as FlatIndex._mask_words: words stay as they are
        (np.uint64 for the host entry, a torch int64 / uint64 device tensor for the device entry), a bool array of length ntotal
        is packed little-endian."""
        if _is_torch(mask):
            import torch
            if mask.dtype == torch.bool:
                pad = (-mask.shape[0]) % 64
                bits = torch.nn.functional.pad(mask.reshape(-1).to(torch.int64), (0, pad)).reshape(-1, 64)
                # (bit 63 wraps into the sign of the int64 word: the same 64 bits)
                return (bits << torch.arange(64, device=mask.device, dtype=torch.int64)).sum(dim=1).contiguous()
            assert mask.dtype in (torch.int64, torch.uint64) and mask.is_cuda == dev
            return mask.reshape(-1).contiguous()
        mask = np.asarray(mask)
        if mask.dtype == np.bool_:
            assert mask.ndim == 1 and mask.shape[0] == self.ntotal, "a bool mask has one entry per insertion index"
            packed = np.packbits(mask, bitorder="little")
            words = np.zeros((mask.shape[0] + 63) // 64 * 8, dtype=np.uint8)
            words[:packed.shape[0]] = packed
            return words.view("<u8").astype(np.uint64, copy=False)
        assert mask.dtype == np.uint64, "a mask is np.uint64 words or a bool array of length ntotal"
        return np.ascontiguousarray(mask.reshape(-1))

    def search_ivf_masked(self, q, nprobe, k, mask, rotate=True, out=None):
        """search_ivf among the entries `mask` allows (cvtmi_opq_search_ivf_masked).  mask: uint64 words, bit i & 63 of word i >> 6
        allowing the entry with INSERTION INDEX i (id - id_base; at least ceil(ntotal / 64) words, bits past ntotal are ignored),
        or a bool array of length ntotal; one mask serves every query.  numpy in (np.uint64 words), numpy out; torch device tensors (int64 / uint64 words) run on
        torch's current stream.  Returns (distances [nq][k] float32, ids [nq][k] int64), padded with (+inf, -1)."""
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            words = self._mask_words(mask, True)
            if out is None:
                d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
                i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            else:
                d, i = out
            _check(lib().cvtmi_opq_search_ivf_masked_dev(self.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(nprobe),
                                                         C.c_int(k), _ptr(words), C.c_int64(words.shape[0]), _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, np.float32)
        words = self._mask_words(mask, False)
        if out is None:
            d = np.empty((nq, k), dtype=np.float32); i = np.empty((nq, k), dtype=np.int64)
        else:
            d, i = out
            assert d.dtype == np.float32 and i.dtype == np.int64 and d.shape == (nq, k) and i.shape == (nq, k)
            assert d.flags.c_contiguous and i.flags.c_contiguous
        _check(lib().cvtmi_opq_search_ivf_masked(self.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(nprobe), C.c_int(k),
                                                 _ptr(words), C.c_int64(words.shape[0]), _ptr(d), _ptr(i)))
        return d, i

    def mask_from_videos(self, video_ids, words=None):
        """The mask of the entries whose video id is in `video_ids` (cvtmi_opq_mask_videos; int32, numpy or a torch device tensor):
        `words` uint64 words (default ceil(ntotal / 64)), every bit past ntotal cleared.  Invert or combine masks with plain word
        operations (~m, a & b)."""
        n_words = (self.ntotal + 63) // 64 if words is None else int(words)
        if _is_torch(video_ids):
            import torch
            assert video_ids.dtype == torch.int32 and video_ids.is_cuda
            video_ids = video_ids.reshape(-1)
            mask = torch.empty(n_words, dtype=torch.int64, device=video_ids.device)
            _check(lib().cvtmi_opq_mask_videos_dev(self.h, _ptr(video_ids), C.c_int64(video_ids.shape[0]), _ptr(mask), C.c_int64(n_words), _stream()))
            return mask
        video_ids = _np(video_ids, np.int32).reshape(-1)
        mask = np.empty(n_words, dtype=np.uint64)
        _check(lib().cvtmi_opq_mask_videos(self.h, _ptr(video_ids), C.c_int64(video_ids.shape[0]), _ptr(mask), C.c_int64(n_words)))
        return mask

    def last_ivf_masked(self):
        """grid of the last search_ivf_masked on this handle (cvtmi_opq_last_ivf_masked)"""
        o = (C.c_int64 * 8)()
        _check(lib().cvtmi_opq_last_ivf_masked(self.h, o))
        return dict(rule=o[0], G=o[1], groups=o[2], pieces=o[3], rows_per_piece=o[4], parts=o[5], part_bytes=o[6], mask_bytes=o[7])

    def range_search_ivf(self, q, nprobe, radius, rotate=True, want_video=False, out=None):
        """Range search (cvtmi_opq_range_search_ivf): every entry of the nprobe nearest coarse lists of a query whose score is
        < radius, in the order of the list-ordered copy.  Returns (lims [nq + 1] int64, distances, ids[, video ids]): the hits of
        query f are [lims[f], lims[f + 1]).
        Without `out` a count-only call sizes the arrays and a second call fills them (torch input: the first one is waited for).
        With out = (lims, dist, ids[, video]) ONE call runs with the capacity of `dist`: numpy raises CvtmiError (code ESPACE)
        when the hits do not fit; torch never waits -- read lims[-1] after synchronising, the arrays are untouched when it is
        larger than their length."""
        nq = q.shape[0]
        dev = _is_torch(q)
        if not dev:
            q = _np(q, np.float32)

        def call(cap, lims, d, i, v):
            args = (self.h, _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(nprobe), C.c_float(float(radius)), C.c_int64(cap),
                    _ptr(lims), _ptr(d), _ptr(i), _ptr(v))
            if dev:
                return lib().cvtmi_opq_range_search_ivf_dev(*args, _stream())
            return lib().cvtmi_opq_range_search_ivf(*args)

        def empty(n, dt):
            if dev:
                import torch
                return torch.empty(n, dtype=getattr(torch, dt), device=q.device)
            return np.empty(n, dtype=dt)

        if out is not None:
            lims, d, i = out[:3]
            v = out[3] if len(out) > 3 else None
            assert lims.shape[0] == nq + 1 and i.shape[0] == d.shape[0] and (v is None or v.shape[0] == d.shape[0])
            _check(call(d.shape[0], lims, d, i, v))
            return out
        lims = empty(nq + 1, "int64")
        _check(call(0, lims, None, None, None))
        total = int(lims[nq])
        d, i = empty(total, "float32"), empty(total, "int64")
        v = empty(total, "int32") if want_video else None
        if total:
            _check(call(total, lims, d, i, v))
        return (lims, d, i, v) if want_video else (lims, d, i)

    def last_range_plan(self):
        """grid of the last range_search_ivf on this handle (cvtmi_opq_last_range_plan)"""
        o = (C.c_int64 * 8)()
        _check(lib().cvtmi_opq_last_range_plan(self.h, o))
        return dict(rule=o[0], G=o[1], groups=o[2], pieces=o[3], rows_per_piece=o[4], parts=o[5], spill=o[6], spill_bytes=o[7])

    def set_param(self, name, value):
        _check(lib().cvtmi_opq_set_param(self.h, name.encode(), C.c_int64(value)))

    def last_mfma(self):
        """(queries, queries the exact scan had to answer) of the last profiled search that took the "scan_mfma" route (cvtmi_opq_last_mfma)"""
        o = (C.c_int64 * 2)()
        _check(lib().cvtmi_opq_last_mfma(self.h, o))
        return int(o[0]), int(o[1])

    def last_scan(self):
        ms = C.c_float(0); b = C.c_int64(0); qt = C.c_int(0); sp = C.c_int(0)
        _check(lib().cvtmi_opq_last_scan(self.h, C.byref(ms), C.byref(b), C.byref(qt), C.byref(sp)))
        return dict(ms=ms.value, code_bytes=b.value, qtile=qt.value, splits=sp.value)


COMM_ID_BYTES = 128
_ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)


class Comm:
    """cvtmi_comm_t: the communicator of the row-sharded search (one process per GPU).

    Comm.unique_id() on rank 0 -> bytes handed to the other ranks by any means -> Comm(id, rank, world) on every
    rank at the same time: RCCL (ncclCommInitRank inside libcvtmi).  Comm.over_torch_group(...) runs the same library
    path over a caller-supplied all-gather (torch.distributed, staged through the host): how several ranks share
    ONE GPU in tests, or what a gloo / MPI job would plug in."""

    def __init__(self, uid, rank, world):
        self.h = C.c_void_p(0)
        self._cb = None
        buf = None
        if uid is not None:
            assert len(uid) == COMM_ID_BYTES
            buf = (C.c_char * COMM_ID_BYTES).from_buffer_copy(bytes(uid))
        _check(lib().cvtmi_comm_create(buf, C.c_int(rank), C.c_int(world), C.byref(self.h)))
        self.rank, self.world = rank, world

    @staticmethod
    def unique_id():
        buf = (C.c_char * COMM_ID_BYTES)()
        _check(lib().cvtmi_comm_unique_id(buf))
        return bytes(buf.raw)

    @classmethod
    def create_all(cls, ndev, devices=None):
        """ONE process driving `ndev` GPUs: ncclCommInitAll inside the library; returns the list of per-device communicators."""
        hs = (C.c_void_p * ndev)()
        dv = None if devices is None else (C.c_int * ndev)(*devices)
        _check(lib().cvtmi_comm_create_all(C.c_int(ndev), dv, hs))
        out = []
        for d in range(ndev):
            self = cls.__new__(cls)
            self.h = C.c_void_p(hs[d]); self._cb = None; self.rank, self.world = d, ndev
            out.append(self)
        return out

    @classmethod
    def custom(cls, fn, rank, world):
        """fn(send_ptr, recv_ptr, nbytes, stream_ptr) -> 0: gather nbytes from every rank into recv (device pointers)."""
        self = cls.__new__(cls)
        self.h = C.c_void_p(0)
        self._cb_error = None

        def guarded(ctx, s, r, nb, st):
            # an exception must not escape a ctypes callback: ctypes would print it and return 0, and the library would merge
            # whatever the gather buffer held (stale lists included) as if the all-gather had happened
            try:
                return int(fn(s, r, nb, st) or 0)
            except BaseException as e:  # noqa: B902 -- KeyboardInterrupt included: re-raised by the caller below
                self._cb_error = e
                return -1

        self._cb = _ALLGATHER_FN(guarded)
        _check(lib().cvtmi_comm_create_custom(self._cb, None, C.c_int(rank), C.c_int(world), C.byref(self.h)))
        self.rank, self.world = rank, world
        return self

    def check(self, rc):
        """_check for calls that may run a caller-supplied all-gather: when that callback raised, the call failed with
        CVTMI_ECOMM -- the callback's own exception is what the caller gets (chained to the library's error)"""
        try:
            _check(rc)
        except CvtmiError as err:
            e, self._cb_error = getattr(self, "_cb_error", None), None
            if e is not None:
                raise e from err
            raise

    def status(self):
        """cvtmi_comm_status: raises CvtmiError (CVTMI_ECOMM) once if a search since the last report failed on some rank under the deferred
        status check (its results were voided: +inf / -1).  Does not synchronise -- synchronise the searches' stream first."""
        _check(lib().cvtmi_comm_status(self.h))

    @classmethod
    def over_torch_group(cls, rank, world, group=None):
        """All-gather through torch.distributed on host buffers (any backend): D2H of this rank's slot, all_gather,
        H2D of everybody's.  The library side (slot layout, merge kernel) is the one the RCCL transport uses."""
        import torch
        import torch.distributed as dist

        def fn(send, recv, nbytes, stream):
            st = torch.cuda.current_stream()
            assert (stream or 0) == st.cuda_stream, "library work was enqueued on another stream than torch's current one"
            st.synchronize()
            hip = C.CDLL("libamdhip64.so")
            mine = torch.empty(nbytes, dtype=torch.uint8)
            if hip.hipMemcpy(C.c_void_p(mine.data_ptr()), C.c_void_p(send), C.c_size_t(nbytes), C.c_int(2)) != 0:
                return 1
            allb = torch.empty(nbytes * world, dtype=torch.uint8)
            dist.all_gather_into_tensor(allb, mine, group=group)
            if hip.hipMemcpy(C.c_void_p(recv), C.c_void_p(allb.data_ptr()), C.c_size_t(nbytes * world), C.c_int(1)) != 0:
                return 1
            return 0

        return cls.custom(fn, rank, world)

    @classmethod
    def over_rendezvous(cls, rv):
        """All-gather staged through the host over a cvt_amd.rendezvous.Rendezvous (plain TCP, no torch.distributed): the
        debug transport that lets several ranks share ONE GPU (bench.py --backend host)."""
        import torch

        def fn(send, recv, nbytes, stream):
            st = torch.cuda.current_stream()
            assert (stream or 0) == st.cuda_stream, "library work was enqueued on another stream than torch's current one"
            st.synchronize()
            hip = C.CDLL("libamdhip64.so")
            mine = (C.c_char * nbytes)()
            if hip.hipMemcpy(mine, C.c_void_p(send), C.c_size_t(nbytes), C.c_int(2)) != 0:
                return 1
            allb = rv.allgather_bytes(mine.raw)
            if len(allb) != nbytes * rv.world:
                return 2
            if hip.hipMemcpy(C.c_void_p(recv), allb, C.c_size_t(len(allb)), C.c_int(1)) != 0:
                return 1
            return 0

        return cls.custom(fn, rv.rank, rv.world)

    def info(self):
        r, w, t = C.c_int(0), C.c_int(0), C.c_int(0)
        n, b = C.c_int64(0), C.c_int64(0)
        _check(lib().cvtmi_comm_info(self.h, C.byref(r), C.byref(w), C.byref(t), C.byref(n), C.byref(b)))
        return {"rank": r.value, "world": w.value, "transport": ("none", "rccl", "custom")[t.value],
                "collectives": n.value, "bytes_per_rank": b.value}

    def merge_topk(self, d, i, k):
        """The exchange step alone for per-shard lists (torch device tensors [nq][k], global ids)."""
        import torch
        nq = d.shape[0]
        od = torch.empty((nq, k), dtype=torch.float32, device=d.device)
        oi = torch.empty((nq, k), dtype=torch.int64, device=d.device)
        self.check(lib().cvtmi_shard_merge_topk_dev(self.h, _ptr(d.contiguous()), _ptr(i.contiguous()), C.c_int64(nq), C.c_int(k),
                                                _ptr(od), _ptr(oi), _stream()))
        return od, oi

    def close(self):
        """Destroys the communicator.  Under the deferred status check (the library default) a rank's failed search voids the
        results (+inf / -1) and leaves the error ON the communicator until the next call or status() collects it: an error nobody
        collected must not vanish with the handle, so close() raises it (after the handle is gone)."""
        if self.h and self.h.value:
            rc = lib().cvtmi_comm_status(self.h)
            msg = lib().cvtmi_last_error().decode(errors="replace") if rc != 0 else ""
            lib().cvtmi_comm_destroy(self.h)
            self.h = C.c_void_p(0)
            if rc != 0:
                raise CvtmiError("cvtmi error %d (uncollected when the communicator was closed): %s" % (rc, msg))

    def __del__(self):
        try:
            self.close()
        except CvtmiError as e:   # nowhere to raise from a finaliser: say it
            import sys
            print("cvt_amd.Comm: %s" % e, file=sys.stderr)
        except Exception:
            pass


def search_sharded_all(indexes, comms, q, k, rotate=True):
    """Single-process multi-GPU search: indexes[d] (OpqIndex or FlatIndex with its id base set) holds the row block of device d,
    comms = Comm.create_all(len(indexes)); q, results: host arrays."""
    nd = len(indexes)
    hs = (C.c_void_p * nd)(*[ix.h.value for ix in indexes])
    cs = (C.c_void_p * nd)(*[c.h.value for c in comms])
    nq = q.shape[0]
    i = np.empty((nq, k), dtype=np.int64)
    if isinstance(indexes[0], FlatIndex):
        q = _np(q, indexes[0]._dt())
        d = np.empty((nq, k), dtype=np.int32 if indexes[0].metric == 2 else np.float32)
        _check(lib().cvtmi_flat_search_sharded_all(hs, cs, C.c_int(nd), _ptr(q), C.c_int64(nq), C.c_int(k), _ptr(d), _ptr(i)))
    else:
        q = _np(q, np.float32)
        d = np.empty((nq, k), dtype=np.float32)
        _check(lib().cvtmi_opq_search_sharded_all(hs, cs, C.c_int(nd), _ptr(q), C.c_int64(nq), C.c_int(1 if rotate else 0), C.c_int(k),
                                                  _ptr(d), _ptr(i)))
    return d, i


def shard_range(n_total, rank, world):
    b, e = C.c_int64(0), C.c_int64(0)
    _check(lib().cvtmi_shard_range(C.c_int64(n_total), C.c_int(rank), C.c_int(world), C.byref(b), C.byref(e)))
    return b.value, e.value


def topk_merge(in_d, in_i, k):
    """[nq][L][k] lists -> [nq][k]"""
    nq, L, kk = in_d.shape
    assert kk == k
    if _is_torch(in_d):
        import torch
        d = torch.empty((nq, k), dtype=torch.float32, device=in_d.device)
        i = torch.empty((nq, k), dtype=torch.int64, device=in_d.device)
        _check(lib().cvtmi_topk_merge_dev(_ptr(in_d), _ptr(in_i), C.c_int64(nq), C.c_int(L), C.c_int(k), _ptr(d),
                                          _ptr(i), _stream()))
        return d, i
    in_d = _np(in_d, np.float32); in_i = _np(in_i, np.int64)
    d = np.empty((nq, k), dtype=np.float32); i = np.empty((nq, k), dtype=np.int64)
    _check(lib().cvtmi_topk_merge(_ptr(in_d), _ptr(in_i), C.c_int64(nq), C.c_int(L), C.c_int(k), _ptr(d), _ptr(i)))
    return d, i


def topk_select(scores, k):
    """scores [nq][n] -> k smallest (score, index) per row; torch device tensors stay on the device (current stream)"""
    if _is_torch(scores):
        import torch
        nq, n = scores.shape
        d = torch.empty((nq, k), dtype=torch.float32, device=scores.device)
        i = torch.empty((nq, k), dtype=torch.int64, device=scores.device)
        _check(lib().cvtmi_topk_select_dev(_ptr(scores), C.c_int64(nq), C.c_int64(n), C.c_int(k), _ptr(d), _ptr(i), _stream()))
        return d, i
    scores = _np(scores, np.float32)
    nq, n = scores.shape
    d = np.empty((nq, k), dtype=np.float32); i = np.empty((nq, k), dtype=np.int64)
    _check(lib().cvtmi_topk_select(_ptr(scores), C.c_int64(nq), C.c_int64(n), C.c_int(k), _ptr(d), _ptr(i)))
    return d, i


class FlatIndex:
    """cvtmi_flat_t: exhaustive search over fp32 (IP, L2) or uint8 (L2) rows."""

    def __init__(self, metric, D):
        self.metric, self.D = metric, D
        self.h = C.c_void_p(0)
        _check(lib().cvtmi_flat_create(C.c_int(metric), C.c_int(D), C.byref(self.h)))

    def close(self):
        if self.h and self.h.value:
            lib().cvtmi_flat_destroy(self.h)
            self.h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _dt(self):
        return np.uint8 if self.metric == 2 else np.float32

    def add(self, x, labels=None):
        if _is_torch(x):
            _check(lib().cvtmi_flat_add_dev(self.h, _ptr(x), _ptr(labels), C.c_int64(x.shape[0]), _stream()))
            return
        x = _np(x, self._dt())
        lab = None if labels is None else _np(labels, np.int64)
        _check(lib().cvtmi_flat_add(self.h, _ptr(x), _ptr(lab), C.c_int64(x.shape[0])))

    @property
    def ntotal(self):
        n = C.c_int64(0)
        _check(lib().cvtmi_flat_ntotal(self.h, C.byref(n)))
        return n.value

    def search(self, q, k):
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            d = torch.empty((nq, k), dtype=torch.int32 if self.metric == 2 else torch.float32, device=q.device)
            i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            _check(lib().cvtmi_flat_search_dev(self.h, _ptr(q), C.c_int64(nq), C.c_int(k), _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, self._dt())
        d = np.empty((nq, k), dtype=np.int32 if self.metric == 2 else np.float32)
        i = np.empty((nq, k), dtype=np.int64)
        _check(lib().cvtmi_flat_search(self.h, _ptr(q), C.c_int64(nq), C.c_int(k), _ptr(d), _ptr(i)))
        return d, i

    def set_id_base(self, base):
        _check(lib().cvtmi_flat_set_id_base(self.h, C.c_int64(base)))

    def remove_labels(self, labels, want_remap=False):
        """Drop every row whose label (what search reports: id_base + row while labels are implicit) is in `labels`
        (cvtmi_flat_remove_labels; int64, numpy or a torch device tensor).  The kept rows close up in their order and keep their
        labels.  Returns the number of rows dropped, with want_remap (dropped, remap): remap[i] = new row of old row i, or -1."""
        n0 = self.ntotal
        removed = C.c_int64(0)
        if _is_torch(labels):
            import torch
            assert labels.dtype == torch.int64 and labels.is_cuda
            labels = labels.reshape(-1)
            remap = torch.empty(n0, dtype=torch.int64, device=labels.device) if want_remap else None
            _check(lib().cvtmi_flat_remove_labels_dev(self.h, _ptr(labels), C.c_int64(labels.shape[0]), C.byref(removed), _ptr(remap), _stream()))
        else:
            labels = _np(labels, np.int64).reshape(-1)
            remap = np.empty(n0, dtype=np.int64) if want_remap else None
            _check(lib().cvtmi_flat_remove_labels(self.h, _ptr(labels), C.c_int64(labels.shape[0]), C.byref(removed), _ptr(remap)))
        return (removed.value, remap) if want_remap else removed.value

    def set_param(self, name, value):
        """cvtmi_flat_set_param: "remove_chunk" = rows the move of a removal works on at a time (0 = default); "range_part_rows" = rows
        per part of a range search (0 = default); "range_spill" = hits a (query, part) may park before the sizes are known (-1 = default);
        "rerank_rows_copy" = 1 lets a rerank build the row-major copy of blocked rows; "masked_parts" = parts per query group of a masked
        search (0 = the plan, 1 .. 1024)."""
        _check(lib().cvtmi_flat_set_param(self.h, name.encode(), C.c_int64(value)))

    def range_search(self, q, radius, out=None):
        """Range search (cvtmi_flat_range_search): every row whose distance to a query is < radius, in ascending row order.  Returns
        (lims [nq + 1] int64, distances (float32; int32 for the uint8 metric), labels): the hits of query f are [lims[f], lims[f + 1]).
        Without `out` a count-only call sizes the arrays and a second call fills them (torch input: the first one is waited for).
        With out = (lims, dist, labels) ONE call runs with the capacity of `dist`: numpy raises CvtmiError (code ESPACE) when the hits
        do not fit; torch never waits -- read lims[-1] after synchronising, the arrays are untouched when it is larger than their
        length."""
        nq = q.shape[0]
        dev = _is_torch(q)
        if not dev:
            q = _np(q, self._dt())
        dist_dt = "int32" if self.metric == 2 else "float32"

        def call(cap, lims, d, i):
            args = (self.h, _ptr(q), C.c_int64(nq), C.c_double(float(radius)), C.c_int64(cap), _ptr(lims), _ptr(d), _ptr(i))
            if dev:
                return lib().cvtmi_flat_range_search_dev(*args, _stream())
            return lib().cvtmi_flat_range_search(*args)

        def empty(n, dt):
            if dev:
                import torch
                return torch.empty(n, dtype=getattr(torch, dt), device=q.device)
            return np.empty(n, dtype=dt)

        if out is not None:
            lims, d, i = out
            assert lims.shape[0] == nq + 1 and i.shape[0] == d.shape[0]
            _check(call(d.shape[0], lims, d, i))
            return out
        lims = empty(nq + 1, "int64")
        _check(call(0, lims, None, None))
        total = int(lims[nq])
        d, i = empty(total, dist_dt), empty(total, "int64")
        if total:
            _check(call(total, lims, d, i))
        return lims, d, i

    def last_range_plan(self):
        """plan of the last range_search on this handle (cvtmi_flat_last_range_plan)"""
        o = (C.c_int64 * 6)()
        _check(lib().cvtmi_flat_last_range_plan(self.h, o))
        return dict(qt=o[0], parts=o[1], rows_per_part=o[2], spill=o[3], spill_bytes=o[4], form=o[5])

    def rerank(self, q, cand, k, cand_base=0):
        """Exact top k among candidate rows (cvtmi_flat_rerank): cand is int64 [nq][R], entry j of query f names row
        cand[f][j] - cand_base; anything outside the index (the -1 padding of the searches, another shard's ids) is skipped and a row
        named twice counts once.  Returns (distances [nq][k] float32 / int32 for the uint8 metric, labels [nq][k] int64) in ascending
        (distance, row) order, padded like search.  numpy in, numpy out; torch device tensors run on torch's current stream."""
        nq, R = cand.shape
        assert q.shape[0] == nq
        if _is_torch(q):
            import torch
            assert _is_torch(cand) and cand.dtype == torch.int64
            d = torch.empty((nq, k), dtype=torch.int32 if self.metric == 2 else torch.float32, device=q.device)
            i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            _check(lib().cvtmi_flat_rerank_dev(self.h, _ptr(q), C.c_int64(nq), _ptr(cand), C.c_int(R), C.c_int64(cand_base), C.c_int(k),
                                               _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, self._dt())
        cand = _np(cand, np.int64)
        d = np.empty((nq, k), dtype=np.int32 if self.metric == 2 else np.float32)
        i = np.empty((nq, k), dtype=np.int64)
        _check(lib().cvtmi_flat_rerank(self.h, _ptr(q), C.c_int64(nq), _ptr(cand), C.c_int(R), C.c_int64(cand_base), C.c_int(k), _ptr(d), _ptr(i)))
        return d, i

    def last_rerank(self):
        """(row source, lanes per distance, workgroups, LDS bytes per workgroup) of the last rerank on this handle
        (cvtmi_flat_last_rerank); row source 0 = row-major primary rows, 1 = blocked rows, 2 = the row-major copy."""
        o = (C.c_int64 * 4)()
        _check(lib().cvtmi_flat_last_rerank(self.h, o))
        return o[0], o[1], o[2], o[3]

    def _mask_words(self, mask, dev):
        """`mask` as uint64 words: words stay as they are, a bool array of length ntotal is packed little-endian (bit r & 63 of word
        r >> 6 = row r)."""
        if _is_torch(mask):
            import torch
            if mask.dtype == torch.bool:
                pad = (-mask.shape[0]) % 64
                bits = torch.nn.functional.pad(mask.reshape(-1).to(torch.int64), (0, pad)).reshape(-1, 64)
                # (bit 63 wraps into the sign of the int64 word: the same 64 bits)
                return (bits << torch.arange(64, device=mask.device, dtype=torch.int64)).sum(dim=1).contiguous()
            assert mask.dtype in (torch.int64, torch.uint64) and mask.is_cuda == dev
            return mask.reshape(-1).contiguous()
        mask = np.asarray(mask)
        if mask.dtype == np.bool_:
            assert mask.ndim == 1 and mask.shape[0] == self.ntotal, "a bool mask has one entry per row"
            packed = np.packbits(mask, bitorder="little")
            words = np.zeros((mask.shape[0] + 63) // 64 * 8, dtype=np.uint8)
            words[:packed.shape[0]] = packed
            return words.view("<u8").astype(np.uint64, copy=False)
        assert mask.dtype == np.uint64, "a mask is np.uint64 words or a bool array of length ntotal"
        return np.ascontiguousarray(mask.reshape(-1))

    def search_masked(self, q, k, mask):
        """The k nearest rows among those `mask` allows (cvtmi_flat_search_masked).  mask: np.uint64 words, bit r & 63 of word r >> 6
        allowing ROW r (at least ceil(ntotal / 64) words; bits past ntotal are ignored), or a bool array of length ntotal; one mask
        serves every query.  Returns (distances [nq][k] float32 / int32 for the uint8 metric, labels [nq][k] int64) in ascending
        (distance, row) order, padded like search when fewer than k rows are allowed.  numpy in, numpy out; torch device tensors
        (mask: int64 / uint64 words or bool) run on torch's current stream."""
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            words = self._mask_words(mask, True)
            assert _is_torch(words) and words.is_cuda
            d = torch.empty((nq, k), dtype=torch.int32 if self.metric == 2 else torch.float32, device=q.device)
            i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            _check(lib().cvtmi_flat_search_masked_dev(self.h, _ptr(q), C.c_int64(nq), C.c_int(k), _ptr(words), C.c_int64(words.shape[0]),
                                                      _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, self._dt())
        words = self._mask_words(mask, False)
        d = np.empty((nq, k), dtype=np.int32 if self.metric == 2 else np.float32)
        i = np.empty((nq, k), dtype=np.int64)
        _check(lib().cvtmi_flat_search_masked(self.h, _ptr(q), C.c_int64(nq), C.c_int(k), _ptr(words), C.c_int64(words.shape[0]), _ptr(d), _ptr(i)))
        return d, i

    def mask_from_labels(self, labels, words=None):
        """The mask of the rows whose reported label is in `labels` (cvtmi_flat_mask_labels; int64, numpy or a torch device tensor):
        `words` uint64 words (default ceil(ntotal / 64)), every bit past ntotal cleared.  Invert or combine masks with plain word
        operations (~m, a & b)."""
        n_words = (self.ntotal + 63) // 64 if words is None else int(words)
        if _is_torch(labels):
            import torch
            assert labels.dtype == torch.int64 and labels.is_cuda
            labels = labels.reshape(-1)
            mask = torch.empty(n_words, dtype=torch.int64, device=labels.device)
            _check(lib().cvtmi_flat_mask_labels_dev(self.h, _ptr(labels), C.c_int64(labels.shape[0]), _ptr(mask), C.c_int64(n_words), _stream()))
            return mask
        labels = _np(labels, np.int64).reshape(-1)
        mask = np.empty(n_words, dtype=np.uint64)
        _check(lib().cvtmi_flat_mask_labels(self.h, _ptr(labels), C.c_int64(labels.shape[0]), _ptr(mask), C.c_int64(n_words)))
        return mask

    def last_masked(self):
        """(queries per workgroup, parts per query group, bytes of the row list, kernel form) of the last search_masked on this handle
        (cvtmi_flat_last_masked); form 0 = fp32 row-major rows, 1 = fp32 blocked rows, 2 = uint8 single bytes, 3 = uint8 16-byte pieces."""
        o = (C.c_int64 * 4)()
        _check(lib().cvtmi_flat_last_masked(self.h, o))
        return o[0], o[1], o[2], o[3]

    def search_sharded(self, comm, q, k):
        """Row-sharded exhaustive search: this handle holds the rank's row block (set_id_base = its first row)."""
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            d = torch.empty((nq, k), dtype=torch.int32 if self.metric == 2 else torch.float32, device=q.device)
            i = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            comm.check(lib().cvtmi_flat_search_sharded_dev(self.h, comm.h, _ptr(q), C.c_int64(nq), C.c_int(k), _ptr(d), _ptr(i), _stream()))
            return d, i
        q = _np(q, self._dt())
        d = np.empty((nq, k), dtype=np.int32 if self.metric == 2 else np.float32)
        i = np.empty((nq, k), dtype=np.int64)
        comm.check(lib().cvtmi_flat_search_sharded(self.h, comm.h, _ptr(q), C.c_int64(nq), C.c_int(k), _ptr(d), _ptr(i)))
        return d, i

    def last_search(self):
        """(how the last search was answered: 0 exact / streaming kernels, 1 sample + matrix-core filter, 2 fp32 stream, 3 fp32 threshold filter, 4 uint8
        threshold filter; largest candidate list (0 for the threshold filters: nothing of theirs is read back))"""
        f = C.c_int(0); m = C.c_int64(0)
        _check(lib().cvtmi_flat_last_search(self.h, C.byref(f), C.byref(m)))
        return f.value, m.value

    def last_redo(self):
        """queries of the last search that the exact kernels answered because the fp32 / uint8 threshold filter or the fp32 stream
        flagged them; -1 when not counted (set_tuning("flat_count_redo", 1) turns counting on; other paths flag nothing: 0)"""
        r = C.c_int64(0)
        _check(lib().cvtmi_flat_last_redo(self.h, C.byref(r)))
        return r.value


class HnswIndex:
    """cvtmi_hnsw_*: batched search over a graph file written by the reference's HierarchicalNSW::saveIndex, or built on the GPU
    (hnsw_build)."""
    def __init__(self, index_bytes, metric, D):
        self.h = C.c_void_p()
        self.D = D
        buf = np.frombuffer(index_bytes, dtype=np.uint8)
        _check(lib().cvtmi_hnsw_load(_ptr(buf), C.c_int64(buf.size), C.c_int(metric), C.c_int(D), C.byref(self.h)))

    def close(self):
        if self.h:
            lib().cvtmi_hnsw_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def save(self):
        """cvtmi_hnsw_save: the reference's saveIndex file of this graph, as bytes"""
        n = C.c_int64(0)
        _check(lib().cvtmi_hnsw_save(self.h, C.c_void_p(0), C.c_int64(0), C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        _check(lib().cvtmi_hnsw_save(self.h, _ptr(buf), C.c_int64(buf.size), C.byref(n)))
        return buf.tobytes()

    @property
    def ntotal(self):
        lib().cvtmi_hnsw_ntotal.restype = C.c_int64
        return int(lib().cvtmi_hnsw_ntotal(self.h))

    def search(self, q, k, ef):
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            assert q.is_contiguous() and q.dtype == torch.float32
            d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            lab = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            _check(lib().cvtmi_hnsw_search_dev(self.h, _ptr(q), C.c_int64(nq), C.c_int(k), C.c_int(ef), _ptr(d), _ptr(lab), _stream()))
            return d, lab
        q = _np(q, np.float32)
        d = np.empty((nq, k), dtype=np.float32); lab = np.empty((nq, k), dtype=np.int64)
        _check(lib().cvtmi_hnsw_search(self.h, _ptr(q), C.c_int64(nq), C.c_int(k), C.c_int(ef), _ptr(d), _ptr(lab)))
        return d, lab

    def search_adc(self, opq, q, k, ef, rotate=True):
        """Same graph, distances = ADC over the PQ codes held by the OpqIndex `opq` (one row per node)."""
        nq = q.shape[0]
        if _is_torch(q):
            import torch
            assert q.is_contiguous() and q.dtype == torch.float32
            d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
            lab = torch.empty((nq, k), dtype=torch.int64, device=q.device)
            _check(lib().cvtmi_hnsw_search_adc_dev(self.h, opq.h, _ptr(q), C.c_int64(nq), C.c_int(int(rotate)), C.c_int(k), C.c_int(ef),
                                                   _ptr(d), _ptr(lab), _stream()))
            return d, lab
        q = _np(q, np.float32)
        d = np.empty((nq, k), dtype=np.float32); lab = np.empty((nq, k), dtype=np.int64)
        _check(lib().cvtmi_hnsw_search_adc(self.h, opq.h, _ptr(q), C.c_int64(nq), C.c_int(int(rotate)), C.c_int(k), C.c_int(ef),
                                           _ptr(d), _ptr(lab)))
        return d, lab


def _hnsw_search_adc_rerank(self, opq, q, k, ef, rerank=None, rotate=True):
    """ADC traversal + exact fp32 re-rank of its `rerank` best nodes (default: ef)."""
    rerank = ef if rerank is None else rerank
    nq = q.shape[0]
    if _is_torch(q):
        import torch
        assert q.is_contiguous() and q.dtype == torch.float32
        d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        lab = torch.empty((nq, k), dtype=torch.int64, device=q.device)
        _check(lib().cvtmi_hnsw_search_adc_rerank_dev(self.h, opq.h, _ptr(q), C.c_int64(nq), C.c_int(int(rotate)), C.c_int(k), C.c_int(ef),
                                                      C.c_int(rerank), _ptr(d), _ptr(lab), _stream()))
        return d, lab
    q = _np(q, np.float32)
    d = np.empty((nq, k), dtype=np.float32); lab = np.empty((nq, k), dtype=np.int64)
    _check(lib().cvtmi_hnsw_search_adc_rerank(self.h, opq.h, _ptr(q), C.c_int64(nq), C.c_int(int(rotate)), C.c_int(k), C.c_int(ef),
                                              C.c_int(rerank), _ptr(d), _ptr(lab)))
    return d, lab


HnswIndex.search_adc_rerank = _hnsw_search_adc_rerank


def _hnsw_mask_words(self, mask, dev):
    """`mask` as uint64 words: words stay as they are, a bool array of length ntotal is packed little-endian (bit i & 63 of word
    i >> 6 = node i)."""
    if _is_torch(mask):
        import torch
        if mask.dtype == torch.bool:
            pad = (-mask.shape[0]) % 64
            bits = torch.nn.functional.pad(mask.reshape(-1).to(torch.int64), (0, pad)).reshape(-1, 64)
            # (bit 63 wraps into the sign of the int64 word: the same 64 bits)
            return (bits << torch.arange(64, device=mask.device, dtype=torch.int64)).sum(dim=1).contiguous()
        assert mask.dtype in (torch.int64, torch.uint64) and mask.is_cuda == dev
        return mask.reshape(-1).contiguous()
    mask = np.asarray(mask)
    if mask.dtype == np.bool_:
        assert mask.ndim == 1 and mask.shape[0] == self.ntotal, "a bool mask has one entry per node"
        packed = np.packbits(mask, bitorder="little")
        words = np.zeros((mask.shape[0] + 63) // 64 * 8, dtype=np.uint8)
        words[:packed.shape[0]] = packed
        return words.view("<u8").astype(np.uint64, copy=False)
    assert mask.dtype == np.uint64, "a mask is np.uint64 words or a bool array of length ntotal"
    return np.ascontiguousarray(mask.reshape(-1))


def _hnsw_masked_call(self, name, head, q, k, mask, tail):
    """One masked entry: `head` / `tail` are the ctypes arguments before the queries and between nq and the mask."""
    nq = q.shape[0]
    if _is_torch(q):
        import torch
        assert q.is_contiguous() and q.dtype == torch.float32
        words = self._mask_words(mask, True)
        assert _is_torch(words) and words.is_cuda
        d = torch.empty((nq, k), dtype=torch.float32, device=q.device)
        lab = torch.empty((nq, k), dtype=torch.int64, device=q.device)
        _check(getattr(lib(), name + "_dev")(self.h, *head, _ptr(q), C.c_int64(nq), *tail, _ptr(words), C.c_int64(words.shape[0]),
                                             _ptr(d), _ptr(lab), _stream()))
        return d, lab
    q = _np(q, np.float32)
    words = self._mask_words(mask, False)
    d = np.empty((nq, k), dtype=np.float32); lab = np.empty((nq, k), dtype=np.int64)
    _check(getattr(lib(), name)(self.h, *head, _ptr(q), C.c_int64(nq), *tail, _ptr(words), C.c_int64(words.shape[0]), _ptr(d), _ptr(lab)))
    return d, lab


def _hnsw_search_masked(self, q, k, ef, mask):
    """search() among the nodes `mask` allows (cvtmi_hnsw_search_masked): hnswlib's filtered searchKnn -- the mask decides what may be
    a result, never what is traversed.  mask: np.uint64 words, bit i & 63 of word i >> 6 allowing NODE i (the insertion order; at
    least ceil(ntotal / 64) words, bits past ntotal are ignored), or a bool array of length ntotal; one mask serves every query.
    Output as search(), padded with (0, -1) when fewer than k allowed nodes are found.  numpy in, numpy out; torch device tensors
    (mask: int64 / uint64 words or bool) run on torch's current stream."""
    return _hnsw_masked_call(self, "cvtmi_hnsw_search_masked", (), q, k, mask, (C.c_int(k), C.c_int(ef)))


def _hnsw_search_adc_masked(self, opq, q, k, ef, mask, rotate=True):
    """search_adc() under a node mask (cvtmi_hnsw_search_adc_masked); mask as in search_masked."""
    return _hnsw_masked_call(self, "cvtmi_hnsw_search_adc_masked", (opq.h,), q, k, mask, (C.c_int(int(rotate)), C.c_int(k), C.c_int(ef)))


def _hnsw_search_adc_rerank_masked(self, opq, q, k, ef, mask, rerank=None, rotate=True):
    """search_adc_rerank() under a node mask (cvtmi_hnsw_search_adc_rerank_masked): the ADC traversal keeps its `rerank` best ALLOWED
    nodes (default: ef), the exact re-rank sees those alone; mask as in search_masked."""
    rerank = ef if rerank is None else rerank
    return _hnsw_masked_call(self, "cvtmi_hnsw_search_adc_rerank_masked", (opq.h,), q, k, mask,
                             (C.c_int(int(rotate)), C.c_int(k), C.c_int(ef), C.c_int(rerank)))


def _hnsw_mask_from_labels(self, labels, words=None):
    """The mask of the nodes whose label is in `labels` (cvtmi_hnsw_mask_labels; int64, numpy or a torch device tensor; uint64 labels
    pass as their int64 bit patterns): `words` uint64 words (default ceil(ntotal / 64)), every bit past ntotal cleared.  Invert or
    combine masks with plain word operations (~m, a & b)."""
    n_words = (self.ntotal + 63) // 64 if words is None else int(words)
    if _is_torch(labels):
        import torch
        assert labels.dtype == torch.int64 and labels.is_cuda
        labels = labels.reshape(-1)
        mask = torch.empty(n_words, dtype=torch.int64, device=labels.device)
        _check(lib().cvtmi_hnsw_mask_labels_dev(self.h, _ptr(labels), C.c_int64(labels.shape[0]), _ptr(mask), C.c_int64(n_words), _stream()))
        return mask
    labels = np.asarray(labels)
    if labels.dtype == np.uint64:
        labels = labels.view(np.int64)
    labels = _np(labels, np.int64).reshape(-1)
    mask = np.empty(n_words, dtype=np.uint64)
    _check(lib().cvtmi_hnsw_mask_labels(self.h, _ptr(labels), C.c_int64(labels.shape[0]), _ptr(mask), C.c_int64(n_words)))
    return mask


def _hnsw_last_masked(self):
    """(slots, candidate-queue capacity per slot in entries, scratch bytes reserved, form) of the last masked search on this handle
    (cvtmi_hnsw_last_masked); form 0 = fp32, 1 = ADC with tables in the scratch, 2 = ADC with tables in LDS."""
    o = (C.c_int64 * 4)()
    _check(lib().cvtmi_hnsw_last_masked(self.h, o))
    return o[0], o[1], o[2], o[3]


HnswIndex._mask_words = _hnsw_mask_words
HnswIndex.search_masked = _hnsw_search_masked
HnswIndex.search_adc_masked = _hnsw_search_adc_masked
HnswIndex.search_adc_rerank_masked = _hnsw_search_adc_rerank_masked
HnswIndex.mask_from_labels = _hnsw_mask_from_labels
HnswIndex.last_masked = _hnsw_last_masked


def _hnsw_add(self, x, labels=None, max_batch=0):
    """cvtmi_hnsw_add[_dev]: the rows x [m][D] (numpy, or a CUDA tensor with labels on the same device) appended as internal ids
    ntotal .. ntotal + m - 1, labels as given (None: the internal ids), batch-synchronous on the GPU as in hnsw_build, the schedule
    continued from the rows the graph holds (max_batch = 1: the reference's sequential addPoint; 0: the default schedule)."""
    m, D = x.shape
    assert D == self.D
    if _is_torch(x):
        import torch
        assert x.is_contiguous() and x.dtype == torch.float32
        lab = None
        if labels is not None:
            lab = labels if _is_torch(labels) else torch.as_tensor(np.ascontiguousarray(labels, dtype=np.uint64).view(np.int64))
            lab = lab.to(device=x.device, dtype=torch.int64).contiguous()
        _check(lib().cvtmi_hnsw_add_dev(self.h, _ptr(x), C.c_int64(m), _ptr(lab), C.c_int(max_batch), _stream()))
        return
    x = _np(x, np.float32)
    lab = None if labels is None else _np(labels, np.uint64)
    _check(lib().cvtmi_hnsw_add(self.h, _ptr(x), C.c_int64(m), _ptr(lab), C.c_int(max_batch)))


def _hnsw_reserve(self, n):
    """cvtmi_hnsw_reserve: the header's max_elements becomes at least n (never lowered)"""
    _check(lib().cvtmi_hnsw_reserve(self.h, C.c_int64(n)))


def _hnsw_level_draws(self):
    """draws taken from the handle's level stream (cvtmi_hnsw_level_draws): n after a build of n rows, 0 after a load, + m per add"""
    n = C.c_int64(0)
    _check(lib().cvtmi_hnsw_level_draws(self.h, C.byref(n)))
    return n.value


def _hnsw_set_level_draws(self, n):
    """cvtmi_hnsw_set_level_draws: the level stream re-seeded and advanced by n draws (n = ntotal after a load: later adds
    continue the build that wrote the file)"""
    _check(lib().cvtmi_hnsw_set_level_draws(self.h, C.c_int64(n)))


def _hnsw_last_add(self):
    """(first internal id, batches, largest batch, max_elements afterwards) of the last add that added rows (cvtmi_hnsw_last_add)"""
    o = (C.c_int64 * 4)()
    _check(lib().cvtmi_hnsw_last_add(self.h, o))
    return o[0], o[1], o[2], o[3]


HnswIndex.add = _hnsw_add
HnswIndex.reserve = _hnsw_reserve
HnswIndex.level_draws = _hnsw_level_draws
HnswIndex.set_level_draws = _hnsw_set_level_draws
HnswIndex.last_add = _hnsw_last_add


def _hnsw_set_deleted(self, name, labels):
    if _is_torch(labels):
        import torch
        assert labels.dtype == torch.int64 and labels.is_cuda
        labels = labels.reshape(-1).contiguous()
        changed = C.c_int64(0)
        _check(getattr(lib(), name + "_dev")(self.h, _ptr(labels), C.c_int64(labels.shape[0]), C.byref(changed), _stream()))
        return changed.value
    labels = np.asarray(labels)
    if labels.dtype == np.uint64:
        labels = labels.view(np.int64)
    labels = _np(labels, np.int64).reshape(-1)
    changed = C.c_int64(0)
    _check(getattr(lib(), name)(self.h, _ptr(labels), C.c_int64(labels.shape[0]), C.byref(changed)))
    return changed.value


def _hnsw_mark_deleted(self, labels):
    """cvtmi_hnsw_mark_deleted[_dev]: hnswlib's markDelete for every node that carries one of `labels` (int64 / uint64, numpy or a
    torch device tensor; duplicates and foreign labels are fine).  A deleted node is still walked through but is never a result, and
    add() links no new row to it; save() keeps the mark (bit 16 of the node's level-0 count word).  Returns the number of nodes
    whose state changed."""
    return _hnsw_set_deleted(self, "cvtmi_hnsw_mark_deleted", labels)


def _hnsw_unmark_deleted(self, labels):
    """cvtmi_hnsw_unmark_deleted[_dev]: the nodes that carry one of `labels` are live again; returns the number that were deleted"""
    return _hnsw_set_deleted(self, "cvtmi_hnsw_unmark_deleted", labels)


def _hnsw_deleted_count(self):
    """deleted nodes of the graph (cvtmi_hnsw_deleted_count)"""
    n = C.c_int64(0)
    _check(lib().cvtmi_hnsw_deleted_count(self.h, C.byref(n)))
    return n.value


def _hnsw_deleted_mask(self, words=None):
    """the delete bitmap (cvtmi_hnsw_get_deleted) as np.uint64 words, bit i & 63 of word i >> 6 = node i is deleted; `words` words
    (default ceil(ntotal / 64)), every bit past ntotal zero"""
    n_words = (self.ntotal + 63) // 64 if words is None else int(words)
    mask = np.empty(n_words, dtype=np.uint64)
    _check(lib().cvtmi_hnsw_get_deleted(self.h, _ptr(mask), C.c_int64(n_words)))
    return mask


HnswIndex.mark_deleted = _hnsw_mark_deleted
HnswIndex.unmark_deleted = _hnsw_unmark_deleted
HnswIndex.deleted_count = _hnsw_deleted_count
HnswIndex.deleted_mask = _hnsw_deleted_mask


def hnsw_build(x, metric, M, ef_construction, labels=None, max_batch=0):
    """cvtmi_hnsw_build[_dev]: a HierarchicalNSW graph over the rows x [n][D] (numpy, or a CUDA tensor with labels on the same
    device), batch-synchronous on the GPU (max_batch = 1: the reference's sequential insertion; 0: the default schedule)."""
    n, D = x.shape
    idx = HnswIndex.__new__(HnswIndex)
    idx.h = C.c_void_p()
    idx.D = D
    if _is_torch(x):
        import torch
        assert x.is_contiguous() and x.dtype == torch.float32
        lab = None
        if labels is not None:
            lab = labels if _is_torch(labels) else torch.as_tensor(np.ascontiguousarray(labels, dtype=np.uint64).view(np.int64))
            lab = lab.to(device=x.device, dtype=torch.int64).contiguous()
        _check(lib().cvtmi_hnsw_build_dev(_ptr(x), C.c_int64(n), C.c_int(D), C.c_int(metric), C.c_int(M), C.c_int(ef_construction),
                                          _ptr(lab), C.c_int(max_batch), C.byref(idx.h), _stream()))
        return idx
    x = _np(x, np.float32)
    lab = None if labels is None else _np(labels, np.uint64)
    _check(lib().cvtmi_hnsw_build(_ptr(x), C.c_int64(n), C.c_int(D), C.c_int(metric), C.c_int(M), C.c_int(ef_construction), _ptr(lab),
                                  C.c_int(max_batch), C.byref(idx.h)))
    return idx


def hnsw_build_phases():
    """[traversal ms, selection ms, back-link ms, batches, host ms] of the last hnsw_build run with set_tuning("hnsw_build_phases", 1)"""
    ms = (C.c_double * 5)()
    _check(lib().cvtmi_hnsw_build_phases(ms))
    return list(ms)


class _PinnedOwner:
    """a cvtmi_host_alloc block; freed when the last numpy view of it goes away (pinned_empty ties the two together)"""

    def __init__(self, nbytes):
        self.p = C.c_void_p(0)
        _check(lib().cvtmi_host_alloc(C.c_size_t(nbytes), C.byref(self.p)))
        self.nbytes = nbytes

    def __del__(self):
        try:
            if self.p and self.p.value:
                lib().cvtmi_host_free(self.p)
                self.p = C.c_void_p(0)
        except Exception:
            pass


def pinned_empty(shape, dtype):
    """numpy array in page-locked host memory (cvtmi_host_alloc): the host-pointer entries move such arrays without a staging
    copy.  The block lives exactly as long as an array views it: the ctypes buffer every view keeps as its base carries the
    owner, so the last view's death frees the page-locked block (no module-level table, nothing leaks)."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    own = _PinnedOwner(max(n, 16))
    buf = (C.c_char * max(n, 16)).from_address(own.p.value)
    buf._cvtmi_owner = own   # numpy keeps `buf` alive as the base of the array and of every view / reshape of it
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    arr.flags.writeable = True
    return arr


def set_tuning(name, value):
    """library-wide tuning / measurement hooks (cvtmi_set_tuning): no effect on results"""
    _check(lib().cvtmi_set_tuning(name.encode(), C.c_int64(int(value))))


def get_tuning(name):
    """the value a cvtmi_set_tuning key holds now (cvtmi_get_tuning): its default, or the last accepted value, normalised"""
    v = C.c_int64(0)
    _check(lib().cvtmi_get_tuning(name.encode(), C.byref(v)))
    return v.value


def kmeans(x, k, niter=0, seed=1):
    """cvtmi_kmeans: (centroids [k][d], assign [n], iterations)."""
    n, d = x.shape
    it = C.c_int(0)
    if _is_torch(x):
        import torch
        assert x.is_contiguous() and x.dtype == torch.float32
        cent = torch.empty((k, d), dtype=torch.float32, device=x.device)
        assign = torch.empty((n,), dtype=torch.int32, device=x.device)
        _check(lib().cvtmi_kmeans_dev(_ptr(x), C.c_int64(d), C.c_int64(n), C.c_int(d), C.c_int(k), C.c_int(niter),
                                      C.c_uint64(seed), _ptr(cent), _ptr(assign), C.byref(it), _stream()))
        return cent, assign, it.value
    x = _np(x, np.float32)
    cent = np.empty((k, d), dtype=np.float32); assign = np.empty(n, dtype=np.int32)
    _check(lib().cvtmi_kmeans(_ptr(x), C.c_int64(n), C.c_int(d), C.c_int(k), C.c_int(niter), C.c_uint64(seed),
                              _ptr(cent), _ptr(assign), C.byref(it)))
    return cent, assign, it.value


def opq_train(x, coarseK, M, K, niter=0, seed=1):
    """cvtmi_opq_train on already permuted / rotated rows: (coarse [coarseK][D], books [M][K][D/M])."""
    n, D = x.shape
    if _is_torch(x):
        import torch
        assert x.is_contiguous() and x.dtype == torch.float32
        coarse = torch.empty((coarseK, D), dtype=torch.float32, device=x.device)
        books = torch.empty((M, K, D // M), dtype=torch.float32, device=x.device)
        _check(lib().cvtmi_opq_train_dev(_ptr(x), C.c_int64(n), C.c_int(D), C.c_int(coarseK), C.c_int(M), C.c_int(K),
                                         C.c_int(niter), C.c_uint64(seed), _ptr(coarse), _ptr(books), _stream()))
        return coarse, books
    x = _np(x, np.float32)
    coarse = np.empty((coarseK, D), dtype=np.float32); books = np.empty((M, K, D // M), dtype=np.float32)
    _check(lib().cvtmi_opq_train(_ptr(x), C.c_int64(n), C.c_int(D), C.c_int(coarseK), C.c_int(M), C.c_int(K), C.c_int(niter),
                                 C.c_uint64(seed), _ptr(coarse), _ptr(books)))
    return coarse, books


def opq_learn_rotation(x, M, K, outer, niter=0, seed=1):
    """cvtmi_opq_learn_rotation: (R [D][D], books [M][K][D/M]) learned from the rows x (numpy -> numpy, torch CUDA -> torch)"""
    n, D = x.shape
    if _is_torch(x):
        import torch
        R = torch.empty((D, D), dtype=torch.float32, device=x.device)
        books = torch.empty((M, K, D // M), dtype=torch.float32, device=x.device)
        _check(lib().cvtmi_opq_learn_rotation_dev(_ptr(x), C.c_int64(n), C.c_int(D), C.c_int(M), C.c_int(K), C.c_int(outer), C.c_int(niter),
                                                  C.c_uint64(seed), _ptr(R), _ptr(books), _stream()))
        return R, books
    x = _np(x, np.float32)
    R = np.empty((D, D), dtype=np.float32); books = np.empty((M, K, D // M), dtype=np.float32)
    _check(lib().cvtmi_opq_learn_rotation(_ptr(x), C.c_int64(n), C.c_int(D), C.c_int(M), C.c_int(K), C.c_int(outer), C.c_int(niter),
                                          C.c_uint64(seed), _ptr(R), _ptr(books)))
    return R, books


def sq8_train(x, l2norm=True):
    n, d = x.shape
    if _is_torch(x):
        import torch
        vmin = torch.empty(d, dtype=torch.float32, device=x.device); vdiff = torch.empty_like(vmin)
        _check(lib().cvtmi_sq8_train_dev(_ptr(x), C.c_int64(n), C.c_int(d), C.c_int(int(l2norm)), _ptr(vmin), _ptr(vdiff),
                                         _stream()))
        return vmin, vdiff
    x = _np(x, np.float32)
    vmin = np.empty(d, dtype=np.float32); vdiff = np.empty(d, dtype=np.float32)
    _check(lib().cvtmi_sq8_train(_ptr(x), C.c_int64(n), C.c_int(d), C.c_int(int(l2norm)), _ptr(vmin), _ptr(vdiff)))
    return vmin, vdiff


def sq8_encode(vmin, vdiff, x, l2norm=True):
    """Returns codes; x is normalised IN PLACE when l2norm is True / 1 (reference behaviour), left alone when l2norm == 2."""
    n, d = x.shape
    if _is_torch(x):
        import torch
        codes = torch.empty((n, d), dtype=torch.uint8, device=x.device)
        _check(lib().cvtmi_sq8_encode_dev(_ptr(vmin), _ptr(vdiff), C.c_int(d), _ptr(x), C.c_int64(n), C.c_int(int(l2norm)),
                                          _ptr(codes), _stream()))
        return codes
    assert x.dtype == np.float32 and x.flags["C_CONTIGUOUS"]
    vmin = _np(vmin, np.float32); vdiff = _np(vdiff, np.float32)
    codes = np.empty((n, d), dtype=np.uint8)
    _check(lib().cvtmi_sq8_encode(_ptr(vmin), _ptr(vdiff), C.c_int(d), _ptr(x), C.c_int64(n), C.c_int(int(l2norm)),
                                  _ptr(codes)))
    return codes


def pca_project(mean, vectors, x, l2norm=True):
    """cvtk::PCAUtils::reduceDim (pca_utils.cc:25-35): (x - mean) * vectors^T, rows L2-normalised.  numpy in ->
    numpy out (host entry); torch CUDA tensors in -> torch tensor out (device entry, current stream)."""
    n, din = x.shape
    dout = vectors.shape[0]
    if _is_torch(x):
        import torch
        y = torch.empty((n, dout), dtype=torch.float32, device=x.device)
        _check(lib().cvtmi_pca_project_dev(_ptr(mean), _ptr(vectors), C.c_int(din), C.c_int(dout), _ptr(x), C.c_int64(n),
                                           C.c_int(1 if l2norm else 0), _ptr(y), _stream()))
        return y
    x = _np(x, np.float32); vectors = _np(vectors, np.float32); mean = _np(mean, np.float32)
    y = np.empty((n, dout), dtype=np.float32)
    _check(lib().cvtmi_pca_project(_ptr(mean), _ptr(vectors), C.c_int(din), C.c_int(dout), _ptr(x), C.c_int64(n),
                                   C.c_int(1 if l2norm else 0), _ptr(y)))
    return y



def pca_covariance(x):
    """cvtmi_pca_covariance: (mean [din] fp32, cov [din][din] float64) of the rows of x, with the arithmetic of
    include/cvtmi.h ("PCA training").  numpy in -> numpy out (host entry); a torch CUDA tensor in -> torch tensors out
    (device entry, current stream)."""
    n, din = x.shape
    if _is_torch(x):
        import torch
        mean = torch.empty(din, dtype=torch.float32, device=x.device)
        cov = torch.empty((din, din), dtype=torch.float64, device=x.device)
        _check(lib().cvtmi_pca_covariance_dev(_ptr(x), C.c_int64(n), C.c_int(din), _ptr(mean), _ptr(cov), _stream()))
        return mean, cov
    x = _np(x, np.float32)
    mean = np.empty(din, dtype=np.float32)
    cov = np.empty((din, din), dtype=np.float64)
    _check(lib().cvtmi_pca_covariance(_ptr(x), C.c_int64(n), C.c_int(din), _ptr(mean), _ptr(cov)))
    return mean, cov


def pca_train(x, dout):
    """cv::PCA(x, noArray(), DATA_AS_ROW, dout) as cvtmi_pca_train computes it: (mean [din], vectors [dout][din],
    values [dout]), the values descending.  numpy in -> numpy out (host entry); a torch CUDA tensor in -> torch tensors
    out (device entry, current stream)."""
    n, din = x.shape
    if _is_torch(x):
        import torch
        mean = torch.empty(din, dtype=torch.float32, device=x.device)
        vectors = torch.empty((dout, din), dtype=torch.float32, device=x.device)
        values = torch.empty(dout, dtype=torch.float32, device=x.device)
        _check(lib().cvtmi_pca_train_dev(_ptr(x), C.c_int64(n), C.c_int(din), C.c_int(dout), _ptr(mean), _ptr(vectors),
                                         _ptr(values), _stream()))
        return mean, vectors, values
    x = _np(x, np.float32)
    mean = np.empty(din, dtype=np.float32)
    vectors = np.empty((max(dout, 0), din), dtype=np.float32)
    values = np.empty(max(dout, 0), dtype=np.float32)
    _check(lib().cvtmi_pca_train(_ptr(x), C.c_int64(n), C.c_int(din), C.c_int(dout), _ptr(mean), _ptr(vectors), _ptr(values)))
    return mean, vectors, values

def sq8_decode(vmin, vdiff, codes):
    n, d = codes.shape
    if _is_torch(codes):
        import torch
        x = torch.empty((n, d), dtype=torch.float32, device=codes.device)
        _check(lib().cvtmi_sq8_decode_dev(_ptr(vmin), _ptr(vdiff), C.c_int(d), _ptr(codes), C.c_int64(n), _ptr(x), _stream()))
        return x
    codes = _np(codes, np.uint8); vmin = _np(vmin, np.float32); vdiff = _np(vdiff, np.float32)
    x = np.empty((n, d), dtype=np.float32)
    _check(lib().cvtmi_sq8_decode(_ptr(vmin), _ptr(vdiff), C.c_int(d), _ptr(codes), C.c_int64(n), _ptr(x)))
    return x


def sq8_decode_faiss(vmin, vdiff, codes):
    """Int8Decode(uint8_t*) / Int8DecodeFaiss arithmetic: the fp32 8-bit codec of faiss (cvtmi_sq8_decode_faiss)"""
    n, d = codes.shape
    if _is_torch(codes):
        import torch
        x = torch.empty((n, d), dtype=torch.float32, device=codes.device)
        _check(lib().cvtmi_sq8_decode_faiss_dev(_ptr(vmin), _ptr(vdiff), C.c_int(d), _ptr(codes), C.c_int64(n), _ptr(x), _stream()))
        return x
    codes = _np(codes, np.uint8); vmin = _np(vmin, np.float32); vdiff = _np(vdiff, np.float32)
    x = np.empty((n, d), dtype=np.float32)
    _check(lib().cvtmi_sq8_decode_faiss(_ptr(vmin), _ptr(vdiff), C.c_int(d), _ptr(codes), C.c_int64(n), _ptr(x)))
    return x
