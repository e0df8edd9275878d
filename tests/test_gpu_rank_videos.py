"""GPU: cvtmi_opq_rank_videos -- Query, the fp32 sum of its rows in frame order and the selection of the best videos, for several
query videos in one call -- against two independent compositions, compared bit for bit:
  (a) the existing entries on the same handle: query_video over all frames, a numpy fp32 fold one frame at a time, topk_select;
  (b) the oracle: orc.query_video + orc.video_rank per segment (finite queries, k <= img_num).
Small model (D = 32, M = 8, K = 64, 16 lists, a permutation as the rotation, 3000 entries with explicit video ids)."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "cvt_amd", "bin")
D, M, K, COARSE_K, N, NPROBE = 32, 8, 64, 16, 3000, 3
K_MAX = 2048
EINVAL = -1
CAP = "ivf_part_cap_mb"


@pytest.fixture(scope="module")
def amd():
    import torch
    torch.cuda.is_available()
    import cvt_amd
    return cvt_amd


class World:
    """model, rows and their codes (encoded once); indexes differ in their video ids only"""

    def __init__(self, amd):
        rng = np.random.default_rng(4951)
        self.amd = amd
        self.coarse = (rng.normal(size=(COARSE_K, D)) * 0.3).astype(np.float32)
        self.books = (rng.normal(size=(M, K, D // M)) * 0.05).astype(np.float32)
        self.perm = rng.permutation(D).astype(np.int32)
        inv = np.argsort(self.perm)
        self.x = (self.coarse[rng.integers(0, COARSE_K, size=N)][:, inv] + 0.05 * rng.normal(size=(N, D))).astype(np.float32)
        idx = amd.OpqIndex(self.coarse, self.books, perm=self.perm)
        self.lists, self.codes = idx.encode(idx.rotate(self.x))
        self.rng = rng

    def index(self, videos):
        idx = self.amd.OpqIndex(self.coarse, self.books, perm=self.perm)
        idx.add_codes(self.codes, self.lists, np.ascontiguousarray(videos, dtype=np.int32))
        return idx

    def frames(self, n, seed):
        rng = np.random.default_rng(seed)
        return (self.x[rng.integers(0, N, size=n)] + 0.01 * rng.normal(size=(n, D))).astype(np.float32)


@pytest.fixture(scope="module")
def world(amd):
    return World(amd)


def seg_offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def fold(ms, seg):
    """total[s] = +0.0; for f ascending: total[s] = total[s] + ms[f], one fp32 add at a time"""
    total = np.zeros((len(seg) - 1, ms.shape[1]), np.float32)
    for s in range(len(seg) - 1):
        for f in range(seg[s], seg[s + 1]):
            total[s] = total[s] + ms[f]
    return total


def reference_a(amd, idx, q, seg, img_num, k, nprobe=NPROBE):
    ms = idx.query_video(q, nprobe, img_num)
    total = fold(ms, seg)
    score, video = amd.topk_select(total, k)
    return score, video, total


def rank(idx, q, seg, img_num, k, want_total, dev, nprobe=NPROBE):
    """rank_videos through the host-pointer or the device-pointer entry, results as numpy"""
    if not dev:
        return idx.rank_videos(q, seg, nprobe, img_num, k, want_total=want_total)
    import torch
    out = idx.rank_videos(torch.from_numpy(q).cuda(), seg, nprobe, img_num, k, want_total=want_total)
    torch.cuda.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def same(got, want, ctx):
    assert np.array_equal(bits(got[0]), bits(want[0])), ("score", ctx)
    assert np.array_equal(got[1], want[1]), ("video", ctx)
    if len(got) > 2:
        assert np.array_equal(bits(got[2]), bits(want[2])), ("total", ctx)


@pytest.mark.parametrize("img_num", [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099])
def test_width_edges(amd, world, orc, img_num):
    """every width the kernel's tiles and its two load forms meet, with img_num equal to the largest video id + 1 and larger; segments of
    1, 0, 9, 2 and 33 frames in one call; with and without the totals; both entries"""
    lengths = [1, 0, 9, 2, 33]
    seg = seg_offsets(lengths)
    q = world.frames(int(seg[-1]), 100 + img_num)
    k = 5
    for ids_below in (img_num, max(1, img_num // 2)):
        videos = world.rng.integers(0, ids_below, size=N)
        videos[0] = ids_below - 1
        idx = world.index(videos)
        want = reference_a(amd, idx, q, seg, img_num, k)
        for s, n in enumerate(lengths):                                   # videos past the entries: exactly the frame count
            assert np.all(want[2][s, ids_below:] == np.float32(n))
        # (b) the oracle, per segment
        off, vid_csr, codes_csr = idx.get_entries()
        oms = orc.query_video(orc.reorder(world.perm, q), world.coarse, world.books, NPROBE, off, codes_csr, vid_csr, img_num)
        kk = min(k, img_num)
        for s in range(len(lengths)):
            if lengths[s] == 0:
                assert np.array_equal(bits(want[2][s]), np.zeros(img_num, np.uint32))
                continue
            ot, od, oi = orc.video_rank(oms[seg[s]:seg[s + 1]], kk)
            assert np.array_equal(bits(ot), bits(want[2][s])), (img_num, s)
            assert np.array_equal(bits(od), bits(want[0][s, :kk])) and np.array_equal(oi, want[1][s, :kk]), (img_num, s)
        for dev in (False, True):
            for want_total in (True, False):
                got = rank(idx, q, seg, img_num, k, want_total, dev)
                same(got, want, (img_num, ids_below, dev, want_total))
        if img_num < k:
            assert np.all(np.isposinf(want[0][:, img_num:])) and np.all(want[1][:, img_num:] == -1)


def test_ties_and_list_lengths(amd, world):
    """k beyond the videos any frame touched: the rest of a list is the smallest untouched ids, all at the frame count exactly;
    k = 1, 128, 129 and 2048 (both selection kernels); k > img_num pads with (+inf, -1)"""
    img_num = 2200
    idx = world.index(world.rng.integers(0, 300, size=N))
    lengths = [4, 1, 7]
    seg = seg_offsets(lengths)
    q = world.frames(int(seg[-1]), 7)
    for k in (1, 128, 129, 2048):
        want = reference_a(amd, idx, q, seg, img_num, k)
        for dev in (False, True):
            same(rank(idx, q, seg, img_num, k, True, dev), want, (k, dev))
            same(rank(idx, q, seg, img_num, k, False, dev), want, (k, dev))
    score, video, total = rank(idx, q, seg, img_num, 2048, True, True)
    for s, n in enumerate(lengths):
        untouched = np.flatnonzero(total[s] == np.float32(n))
        touched = img_num - untouched.size
        assert 0 < touched < 400 and np.all(total[s, 300:] == np.float32(n))
        assert np.all(score[s, :touched] < np.float32(n)) and np.all(np.diff(score[s]) >= 0)
        assert np.array_equal(video[s, touched:], untouched[:2048 - touched])      # ties go to the smaller video id
        assert np.all(score[s, touched:] == np.float32(n))
    idx63 = world.index(world.rng.integers(0, 63, size=N))
    for dev in (False, True):
        got = rank(idx63, q, seg, 63, 100, True, dev)
        same(got, reference_a(amd, idx63, q, seg, 63, 100), dev)
        assert np.all(np.isposinf(got[0][:, 63:])) and np.all(got[1][:, 63:] == -1)
        assert np.all(np.isfinite(got[0][:, :63])) and np.all(got[1][:, :63] >= 0)


def test_chunk_cuts(amd, world):
    """one frame per chunk (cap 0), and a cap of 1 MB at 40 000 videos -- six frames per chunk, the cuts inside segments: the same bits
    as under the default cap, and last_rank reports the chunks"""
    before = amd.get_tuning(CAP)
    cases = [(0, 257, [1, 0, 9, 2, 33], 1), (1, 40000, [4, 9, 1, 0, 7], (1 << 20) // (40000 * 4))]
    try:
        for cap, img_num, lengths, per_chunk in cases:
            idx = world.index(world.rng.integers(0, img_num, size=N))
            seg = seg_offsets(lengths)
            frames = int(seg[-1])
            q = world.frames(frames, 11 + cap)
            amd.set_tuning(CAP, before)
            want = reference_a(amd, idx, q, seg, img_num, 9)
            for dev in (False, True):
                same(rank(idx, q, seg, img_num, 9, True, dev), want, ("default", img_num, dev))
            last = idx.last_rank()
            assert last["chunks"] == 1 and last["frames_per_chunk"] == frames and last["total_bytes"] == 0, last
            amd.set_tuning(CAP, cap)
            for dev in (False, True):
                for want_total in (True, False):
                    same(rank(idx, q, seg, img_num, 9, want_total, dev), want, (cap, img_num, dev, want_total))
                    last = idx.last_rank()
                    assert last["frames_per_chunk"] == per_chunk and last["score_bytes"] == per_chunk * img_num * 4, last
                    if want_total:                                         # all segments in one group: the chunks run over the whole frame list
                        assert last["chunks"] == -(-frames // per_chunk) > 1 and last["total_bytes"] == 0, last
                    else:
                        assert last["chunks"] > 1 and last["total_bytes"] > 0, last
    finally:
        amd.set_tuning(CAP, before)


def test_segment_groups(amd, world):
    """total == NULL under a cap of 0: one segment per group, each selected before the next begins -- the lists of the call that was given
    its totals"""
    before = amd.get_tuning(CAP)
    img_num = 1025
    idx = world.index(world.rng.integers(0, img_num, size=N))
    seg = seg_offsets([5, 3, 6])
    q = world.frames(14, 21)
    want = rank(idx, q, seg, img_num, 12, True, False)
    same(want, reference_a(amd, idx, q, seg, img_num, 12), "default")
    try:
        amd.set_tuning(CAP, 0)
        for dev in (False, True):
            got = rank(idx, q, seg, img_num, 12, False, dev)
            same(got, want[:2], dev)
            last = idx.last_rank()
            assert last["total_bytes"] == img_num * 4 and last["chunks"] == 14 and last["frames_per_chunk"] == 1, last
    finally:
        amd.set_tuning(CAP, before)


def test_total_is_written_in_full(amd, world):
    """the caller's totals are never read: NaN bit patterns in every cell beforehand, every cell -- the empty segment's too -- written"""
    import torch
    img_num = 257
    idx = world.index(world.rng.integers(0, img_num, size=N))
    lengths = [3, 0, 5]
    seg = seg_offsets(lengths)
    q = world.frames(8, 31)
    want = reference_a(amd, idx, q, seg, img_num, 4)
    lib = amd.lib()
    args = (C.c_int64(3), C.c_int(1), C.c_int(NPROBE), C.c_int(img_num), C.c_int(4))
    score = np.empty((3, 4), np.float32); video = np.empty((3, 4), np.int64)
    total = np.full((3, img_num), 0x7fc01234, np.uint32).view(np.float32)
    assert lib.cvtmi_opq_rank_videos(idx.h, q.ctypes.data_as(C.c_void_p), seg.ctypes.data_as(C.c_void_p), *args, score.ctypes.data_as(C.c_void_p),
                                     video.ctypes.data_as(C.c_void_p), total.ctypes.data_as(C.c_void_p)) == 0
    same((score, video, total), want, "host")
    assert np.array_equal(bits(total[1]), np.zeros(img_num, np.uint32))
    qd = torch.from_numpy(q).cuda()
    sd = torch.empty((3, 4), dtype=torch.float32, device="cuda"); vd = torch.empty((3, 4), dtype=torch.int64, device="cuda")
    td = torch.from_numpy(np.full((3, img_num), 0x7fc01234, np.uint32).view(np.float32)).cuda()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.cvtmi_opq_rank_videos_dev(idx.h, C.c_void_p(qd.data_ptr()), seg.ctypes.data_as(C.c_void_p), *args, C.c_void_p(sd.data_ptr()),
                                         C.c_void_p(vd.data_ptr()), C.c_void_p(td.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    same((sd.cpu().numpy(), vd.cpu().numpy(), td.cpu().numpy()), want, "device")


def test_nan_frame(amd, world):
    """a NaN in the middle frame of one segment: totals and lists as composition (a) gives them; the other segment of the call is
    what it is without the NaN"""
    img_num = 256
    idx = world.index(world.rng.integers(0, img_num, size=N))
    seg = seg_offsets([3, 4])
    q = world.frames(7, 41)
    clean = rank(idx, q, seg, img_num, 10, True, False)
    q[1, 5] = np.nan
    want = reference_a(amd, idx, q, seg, img_num, 10)
    assert np.isnan(want[2][0]).any() and not np.isnan(want[2][0]).all() and not np.isnan(want[2][1]).any()
    for dev in (False, True):
        for want_total in (True, False):
            got = rank(idx, q, seg, img_num, 10, want_total, dev)
            same(got, want, (dev, want_total))
            same(tuple(g[1:] for g in got), tuple(c[1:] for c in clean[:len(got)]), "the finite segment")


def test_argument_checks(amd, world):
    img_num = 64
    idx = world.index(world.rng.integers(0, img_num, size=N))
    q = world.frames(6, 51)
    ok = seg_offsets([2, 4])

    def fails(seg=ok, nprobe=NPROBE, img=img_num, k=3):
        for dev in (False, True):
            with pytest.raises(amd.CvtmiError) as e:
                rank(idx, q, np.asarray(seg, np.int64), img, k, False, dev, nprobe=nprobe)
            assert e.value.code == EINVAL, (e.value, dev)

    fails(seg=[0, 4, 2])                    # decreasing
    fails(seg=[1, 2, 6])                    # seg_off[0] != 0
    fails(k=0)
    fails(k=K_MAX + 1)
    fails(img=0)
    fails(nprobe=0)
    # a video id >= img_num: CVTMI_EINVAL, the outputs untouched
    lib = amd.lib()
    score = np.full((2, 3), 7, np.float32); video = np.full((2, 3), 7, np.int64); total = np.full((2, img_num - 1), 7, np.float32)
    rc = lib.cvtmi_opq_rank_videos(idx.h, q.ctypes.data_as(C.c_void_p), ok.ctypes.data_as(C.c_void_p), C.c_int64(2), C.c_int(1), C.c_int(NPROBE),
                                   C.c_int(img_num - 1), C.c_int(3), score.ctypes.data_as(C.c_void_p), video.ctypes.data_as(C.c_void_p),
                                   total.ctypes.data_as(C.c_void_p))
    assert rc == EINVAL and b"outside img_num" in lib.cvtmi_last_error()
    assert np.all(score == 7) and np.all(video == 7) and np.all(total == 7)
    # nseg == 0: OK, nothing written
    rc = lib.cvtmi_opq_rank_videos(idx.h, None, ok.ctypes.data_as(C.c_void_p), C.c_int64(0), C.c_int(1), C.c_int(NPROBE), C.c_int(img_num), C.c_int(3),
                                   score.ctypes.data_as(C.c_void_p), video.ctypes.data_as(C.c_void_p), total.ctypes.data_as(C.c_void_p))
    assert rc == 0 and np.all(score == 7) and np.all(video == 7) and np.all(total == 7)
    s, v = idx.rank_videos(q[:0], [0], NPROBE, img_num, 3)
    assert s.shape == (0, 3) and v.shape == (0, 3)


def test_two_threads_on_one_handle(amd, world):
    """rankings with different segmentations side by side on one handle: each thread gets what it gets alone"""
    img_num = 1023
    idx = world.index(world.rng.integers(0, img_num, size=N))
    jobs = [(seg_offsets([9, 2, 0, 5]), world.frames(16, 61), 7), (seg_offsets([1, 12, 3, 3, 4]), world.frames(23, 62), 130)]
    alone = [rank(idx, q, seg, img_num, k, True, False) for seg, q, k in jobs]
    got = [[], []]
    errors = []

    def work(j):
        try:
            seg, q, k = jobs[j]
            for _ in range(4):
                got[j].append(rank(idx, q, seg, img_num, k, True, False))
        except Exception as e:   # noqa: BLE001 -- reported by the assertion below
            errors.append(e)

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for j in range(2):
        assert len(got[j]) == 4
        for g in got[j]:
            same(g, alone[j], j)


def test_opq_query_batch_writes_what_the_loop_writes(tmp_path):
    """opq_query --batch (IVFOPQ::QueryRank, one cvtmi_opq_rank_videos call) against the loop: result.txt and stdout byte for byte;
    three query files, one of them empty"""
    from oracle import binding as ob
    rng = np.random.default_rng(29)
    nv, coarse_k, m = 9, 6, 4
    coarse = (rng.normal(size=(coarse_k, D)) * 0.3).astype(np.float32)
    books = (rng.normal(size=(m, K, D // m)) * 0.05).astype(np.float32)
    perm = rng.permutation(D).astype(np.int32)
    inv = np.argsort(perm)
    vids = [(coarse[v % coarse_k][inv] + 0.05 * rng.normal(size=(int(rng.integers(2, 6)), D))).astype(np.float32) for v in range(nv)]
    names = []
    for v, x in enumerate(vids):
        f = tmp_path / ("v%04d_feat.bin" % v)
        x.tofile(f)
        names.append(str(f))
    (tmp_path / "list.txt").write_text("\n".join(names) + "\n")
    model = str(tmp_path / "model.bin")
    ob.write_opq_model(model, coarse, books, perm)
    (tmp_path / "idx").mkdir()

    def run(args):
        r = subprocess.run(args, cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-2000:])
        return r.stdout

    run([os.path.join(BIN, "opq_index"), model, str(tmp_path / "list.txt"), str(tmp_path / "idx"), str(nv)])
    idx_file = str(tmp_path / "idx" / os.listdir(tmp_path / "idx")[0])
    (np.stack([vids[1][0], vids[4][-1], vids[7][0]]).astype(np.float32) + np.float32(0.01)).tofile(tmp_path / "q0.bin")
    (tmp_path / "q1.bin").write_bytes(b"")
    (vids[3] + np.float32(0.02)).astype(np.float32).tofile(tmp_path / "q2.bin")
    queries = [str(tmp_path / n) for n in ("q0.bin", "q1.bin", "q2.bin")]
    for show in (3, 13):                                                   # 13 > 9 videos: the entries past them are (0, 0)
        common = [os.path.join(BIN, "opq_query"), model, idx_file]
        loop = run(common + [str(tmp_path / "loop.txt")] + queries + ["--nearest", "2", "--show", str(show)])
        batch = run(common + [str(tmp_path / "batch.txt")] + queries + ["--nearest", "2", "--show", str(show), "--batch"])
        assert batch == loop
        assert (tmp_path / "batch.txt").read_bytes() == (tmp_path / "loop.txt").read_bytes()
        assert loop.count("query ID:") == 3 and "query ID: 1, frame_num:0" in loop and len((tmp_path / "loop.txt").read_text()) > 0
