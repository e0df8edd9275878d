// bf_masked_check -- self-check of hnswlib::BruteforceSearch::searchKnn(query, k, BaseFilterFunctor *) and the filtered
// searchKnnBatch (cvt_amd/host/hnswlib/bruteforce.h, an extension with current hnswlib's signature: the reference has no filter).
// The answer of the device (cvtmi_flat_mask_labels + cvtmi_flat_search_masked) must be exactly the k smallest (distance, label)
// pairs of a host loop over the ALLOWED rows with the space's own distance function -- same distances, bit for bit, same order --
// for the float spaces (inner product, L2) and the int space, under filters that keep every label, none, one, every third and a
// cluster at the end of the label range, at k below, at and above the number of allowed rows; also after removePoint and with
// labels added out of order.  A NULL functor must be the unfiltered call.  Prints "OK" and returns 0, or the first difference.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../hnswlib/hnswlib.h"

using namespace hnswlib;

struct Filter : BaseFilterFunctor {
    int mode;
    labeltype a;
    size_t calls;
    Filter(int m, labeltype v) : mode(m), a(v), calls(0) {}
    bool operator()(labeltype l)
    {
        ++calls;
        switch (mode) {
            case 0: return true;            // every label
            case 1: return false;           // none
            case 2: return l == a;          // one
            case 3: return l % 3 == 0;      // every third
            default: return l >= a;         // a cluster at the end
        }
    }
};

template <typename dist_t>
static bool check(BruteforceSearch<dist_t> &idx, const void *q, size_t k, Filter *f, const char *what)
{
    // the expectation: the host distance loop over the allowed rows of data_, the k smallest (distance, label)
    std::vector<std::pair<dist_t, labeltype> > want;
    for (size_t i = 0; i < idx.cur_element_count; ++i) {
        const char *row = idx.data_ + idx.size_per_element_ * i;
        const labeltype lab = *(const labeltype *)(row + idx.data_size_);
        if (f && !(*f)(lab)) continue;
        want.push_back(std::make_pair(idx.fstdistfunc_(q, row, idx.dist_func_param_), lab));
    }
    std::sort(want.begin(), want.end());
    if (want.size() > k) want.resize(k);
    if (f) f->calls = 0;
    std::vector<dist_t> d(k);
    std::vector<int64_t> l(k);
    idx.searchKnnBatch(q, 1, k, d.data(), l.data(), f);
    if (f && f->calls != idx.cur_element_count) {
        printf("MISMATCH %s mode %d: the functor ran %zu times for %zu labels\n", what, f->mode, f->calls, idx.cur_element_count);
        return false;
    }
    for (size_t i = 0; i < k; ++i) {
        const bool pad = i >= want.size();
        if (pad ? l[i] != -1 : (l[i] != (int64_t)want[i].second || memcmp(&d[i], &want[i].first, sizeof(dist_t)) != 0)) {
            printf("MISMATCH %s mode %d k %zu: entry %zu: (%g, %lld) vs %s(%g, %zu)\n", what, f ? f->mode : -1, k, i, (double)d[i], (long long)l[i],
                   pad ? "padding " : "", pad ? 0.0 : (double)want[i].first, pad ? (size_t)0 : (size_t)want[i].second);
            return false;
        }
    }
    // the single-query form returns the same entries through the reference's heap
    std::priority_queue<std::pair<dist_t, labeltype> > top = idx.searchKnn(const_cast<void *>(q), k, f);
    if (top.size() != want.size()) {
        printf("MISMATCH %s mode %d k %zu: searchKnn returned %zu entries, expected %zu\n", what, f ? f->mode : -1, k, top.size(), want.size());
        return false;
    }
    for (size_t i = want.size(); i-- > 0; top.pop())
        if (top.top().second != want[i].second || memcmp(&top.top().first, &want[i].first, sizeof(dist_t)) != 0) {
            printf("MISMATCH %s mode %d k %zu: searchKnn entry %zu\n", what, f ? f->mode : -1, k, i);
            return false;
        }
    return true;
}

// every filter at k below, at and above what it allows
template <typename dist_t>
static bool filters(BruteforceSearch<dist_t> &idx, const void *q, labeltype one, labeltype tail, const char *what)
{
    size_t third = 0, last = 0;
    for (size_t i = 0; i < idx.cur_element_count; ++i) {
        const labeltype lab = *(const labeltype *)(idx.data_ + idx.size_per_element_ * i + idx.data_size_);
        third += lab % 3 == 0;
        last += lab >= tail;
    }
    Filter all(0, 0), none(1, 0), single(2, one), every3(3, 0), cluster(4, tail);
    const size_t ks[] = { 1, 10, 129 };
    for (size_t k : ks)
        if (!check<dist_t>(idx, q, k, &all, what) || !check<dist_t>(idx, q, k, &none, what) || !check<dist_t>(idx, q, k, &single, what) ||
            !check<dist_t>(idx, q, k, &every3, what) || !check<dist_t>(idx, q, k, &cluster, what) || !check<dist_t>(idx, q, k, NULL, what))
            return false;
    return check<dist_t>(idx, q, third, &every3, what) && check<dist_t>(idx, q, third + 1, &every3, what) && check<dist_t>(idx, q, last - 1, &cluster, what) &&
           check<dist_t>(idx, q, last, &cluster, what) && check<dist_t>(idx, q, last + 1, &cluster, what);
}

int main()
{
    const size_t n = 1025;   // two 512-entry search tiles and one row
    std::mt19937 rng(29);
    {   // float spaces: L2 at a blocked width, inner product at a blocked and at a row-major one
        for (int pass = 0; pass < 3; ++pass) {
            const size_t dim = pass == 0 ? 64 : pass == 1 ? 20 : 37;
            L2Space l2(dim);
            InnerProductSpace ip(dim);
            SpaceInterface<float> *space = pass == 0 ? (SpaceInterface<float> *)&l2 : (SpaceInterface<float> *)&ip;
            std::normal_distribution<float> g(0.f, 1.f);
            BruteforceSearch<float> idx(space, n + 8);
            std::vector<float> first(dim), r(dim);
            for (size_t i = 0; i < n; ++i) {
                for (auto &v : r) v = g(rng);
                if (i == 0) first = r;
                if (i % 7 == 3) r = first;                                   // exact duplicates: ties across the filter
                idx.addPoint(r.data(), (labeltype)(i < 900 ? 2 * i : 2 * (i - 900) + 1));   // the last rows interleave: a re-sort by label
            }
            std::vector<float> q(dim);
            for (auto &v : q) v = g(rng);
            const char *what = pass == 0 ? "L2 64-d" : pass == 1 ? "IP 20-d" : "IP 37-d";
            if (!filters<float>(idx, q.data(), 6, 1500, what) || !filters<float>(idx, first.data(), 20, 1700, what)) return 1;
            for (int t = 0; t < 9; ++t) idx.removePoint((labeltype)(2 * (50 + 40 * t)));   // dropped on the device
            idx.removePoint(0);                                                           // the row every duplicate copies
            if (!filters<float>(idx, first.data(), 6, 1500, what)) return 1;
        }
    }
    {   // the int space: 32 bytes (16-byte pieces) and 5 (single bytes, the tail byte dropped)
        for (int pass = 0; pass < 2; ++pass) {
            const size_t dim = pass == 0 ? 32 : 5;
            L2SpaceI space(dim);
            BruteforceSearch<int> idx(&space, n + 8);
            std::vector<unsigned char> first(dim), r(dim);
            for (size_t i = 0; i < n; ++i) {
                for (auto &v : r) v = (unsigned char)(rng() & 255);
                if (i == 0) first = r;
                if (i % 7 == 3) r = first;
                idx.addPoint(r.data(), (labeltype)(3 * i + (i & 1)));
            }
            std::vector<unsigned char> q(dim);
            for (auto &v : q) v = (unsigned char)(rng() & 255);
            const char *what = pass == 0 ? "L2I 32-d" : "L2I 5-d";
            if (!filters<int>(idx, q.data(), 6, 2900, what) || !filters<int>(idx, first.data(), 30, 3000, what)) return 1;
            idx.removePoint(0);
            idx.removePoint(3 * 700);
            if (!filters<int>(idx, first.data(), 6, 2900, what)) return 1;
        }
    }
    printf("OK\n");
    return 0;
}
