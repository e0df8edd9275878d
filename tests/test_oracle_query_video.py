"""CPU: orc_query_video (the checker of cvtmi_opq_query_video) against the reference's own QueryThrehold run live
(oracle/_ref/libref_opq.so), at the cases where a restatement of IVFOPQ.cpp:322-422 can drift from it: non-finite
frames (std::min lets a NaN score replace its cell), ties at the nk-th probe, nk = coarseK, and widths that are not
multiples of 16."""
import numpy as np
import pytest

from conftest import bits

from oracle import binding as ob

pytestmark = pytest.mark.skipif(not ob.ref_available(), reason="oracle/_ref not built")


def same_scores(a, b):
    """Bits on cells that are not NaN, NaN-ness (not the payload) on the others."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0, a)), bits(np.where(nb, 0, b)))


def _grid(x, step=2.0 ** -12):
    return (np.round(np.asarray(x, np.float64) / step) * step).astype(np.float32)


def _case(D, M, L, n_videos, seed):
    """coarseK = L lists on a 2^-12 grid (so that p +- e and its differences are exact) with two ties built in:
    list 7 duplicated as list L - 5, and lists 10 / L - 3 equidistant from a point p.  Video v holds rows around
    list v % L, the duplicated and equidistant lists included."""
    rng = np.random.default_rng(seed)
    coarse = _grid(rng.normal(size=(L, D)) * 0.3)
    coarse[L - 5] = coarse[7]
    p = _grid(rng.normal(size=D) * 0.3)
    e = _grid(rng.normal(size=D) * 0.02)
    coarse[10], coarse[L - 3] = p + e, p - e
    books = (rng.normal(size=(M, 256, D // M)) * 0.01).astype(np.float32)
    perm = rng.permutation(D).astype(np.int32)
    inv = np.argsort(perm)
    centres = [7, 10, L - 3] + [int(c) for c in rng.integers(0, L, size=n_videos - 3)]
    vids = [(coarse[c][inv] + 0.003 * rng.normal(size=(int(rng.integers(3, 9)), D))).astype(np.float32) for c in centres]
    return rng, coarse, books, perm, inv, p, vids


def _frames(rng, coarse, inv, p, vids, D):
    """Raw (un-rotated) frames: ordinary ones near the data, then the edge cases."""
    q = [v[0] + 0.002 * rng.normal(size=D).astype(np.float32) for v in vids[:4]]
    nan = np.array(q[0]); nan[D // 3] = np.nan
    nneg = np.array(q[1]); nneg[0] = -np.nan                            # NaN with the sign bit set
    q += [nan, nneg]
    q += [np.full(D, np.inf, np.float32), np.full(D, 1e30, np.float32)]
    q += [coarse[7][inv], p[inv]]                                     # on the duplicated centroid; the midpoint
    q = np.stack(q).astype(np.float32)
    assert np.signbit(q[5, 0]) and np.isnan(q[5, 0])
    return q


@pytest.mark.parametrize("D,M,L", [(64, 8, 64), (36, 4, 48)], ids=["d64m8", "d36m4"])
def test_query_video_matches_reference_at_the_edges(orc, D, M, L):
    n_videos = 12
    rng, coarse, books, perm, inv, p, vids = _case(D, M, L, n_videos, 1000 + D)
    q = _frames(rng, coarse, inv, p, vids, D)
    ref = ob.RefOPQ(coarse, books, perm)
    try:
        assert ref.index(vids) == n_videos
        off, vid, codes = ref.dump()
        qr = orc.reorder(perm, q)
        for nk in (1, 2, 3, L):                                          # 1, 2: the boundary inside the tied pairs
            rms = ref.query(q, nk, n_videos)
            oms = orc.query_video(qr, coarse, books, nk, off, codes, vid, n_videos)
            assert same_scores(oms, rms), nk
            # the NaN frames: NaN in every video met in the probed lists (the first nk lists), whatever the sign of the NaN
            met = np.zeros(n_videos, bool)
            met[vid[off[0]:off[nk]]] = True
            for f in (4, 5):
                assert np.array_equal(np.isnan(rms[f]), met), (nk, f)
                assert np.all(oms[f][~met] == 1.0)
            # +inf and 1e30 frames: every distance overflows, every score stays at the 1.0 clamp
            assert np.all(rms[6:8] == 1.0)
        # the ties decide something: list 7 and its copy, lists 10 and L - 3, hold different videos
        assert off[8] > off[7] and off[11] > off[10] and off[L - 2] > off[L - 3]
        assert off[L - 4] == off[L - 5]                                  # the copy of list 7 is never chosen by Add
    finally:
        ref.close()
