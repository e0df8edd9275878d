// bf_range_check -- self-check of hnswlib::BruteforceSearch::searchRange (cvt_amd/host/hnswlib/bruteforce.h, an extension: the
// reference has no range query).  The hits of the device (cvtmi_flat_range_search) must be exactly the rows whose distance, taken
// with the space's own host distance function, is under the radius -- same distances, bit for bit, in ascending label order -- for
// a float space and the int space, at radii that are distances of the table (strict: that row is out), just above them, zero and
// huge; also after removePoint and with labels added out of order.  Prints "OK" and returns 0, or the first difference.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "../hnswlib/hnswlib.h"

using namespace hnswlib;

template <typename dist_t>
static bool check(BruteforceSearch<dist_t> &idx, const void *q, dist_t radius, const char *what)
{
    // the expectation: the host distance loop over data_, sorted by label
    std::vector<std::pair<labeltype, dist_t> > want;
    for (size_t i = 0; i < idx.cur_element_count; ++i) {
        const char *row = idx.data_ + idx.size_per_element_ * i;
        const dist_t d = idx.fstdistfunc_(q, row, idx.dist_func_param_);
        if (d < radius) want.push_back(std::make_pair(*(const labeltype *)(row + idx.data_size_), d));
    }
    std::sort(want.begin(), want.end());
    const std::vector<std::pair<dist_t, labeltype> > got = idx.searchRange(q, radius);
    if (got.size() != want.size()) {
        printf("MISMATCH %s radius %g: %zu hits, expected %zu\n", what, (double)radius, got.size(), want.size());
        return false;
    }
    for (size_t i = 0; i < got.size(); ++i)
        if (got[i].second != want[i].first || memcmp(&got[i].first, &want[i].second, sizeof(dist_t)) != 0) {
            printf("MISMATCH %s radius %g: hit %zu: (%g, %zu) vs (%g, %zu)\n", what, (double)radius, i, (double)got[i].first, (size_t)got[i].second,
                   (double)want[i].second, (size_t)want[i].first);
            return false;
        }
    return true;
}

// the radii of one query: the distance of row `pick` (strict: out), the next value above it (in), zero, and everything
static bool radii(BruteforceSearch<float> &idx, const float *q, size_t pick, const char *what)
{
    const float d = idx.fstdistfunc_(q, idx.data_ + idx.size_per_element_ * pick, idx.dist_func_param_);
    return check<float>(idx, q, d, what) && check<float>(idx, q, std::nextafter(d, std::numeric_limits<float>::infinity()), what) &&
           check<float>(idx, q, 0.0f, what) && check<float>(idx, q, std::numeric_limits<float>::infinity(), what);
}
static bool radii(BruteforceSearch<int> &idx, const unsigned char *q, size_t pick, const char *what)
{
    const int d = idx.fstdistfunc_(q, idx.data_ + idx.size_per_element_ * pick, idx.dist_func_param_);
    return check<int>(idx, q, d, what) && check<int>(idx, q, d + 1, what) && check<int>(idx, q, 0, what) &&
           check<int>(idx, q, std::numeric_limits<int>::max(), what);
}

int main()
{
    const size_t n = 1025;   // four 256-row tiles and one row
    std::mt19937 rng(23);
    {   // float spaces: L2 at a blocked width, inner product at a row-major one
        for (int pass = 0; pass < 2; ++pass) {
            const size_t dim = pass == 0 ? 64 : 37;
            L2Space l2(dim);
            InnerProductSpace ip(dim);
            SpaceInterface<float> *space = pass == 0 ? (SpaceInterface<float> *)&l2 : (SpaceInterface<float> *)&ip;
            std::normal_distribution<float> g(0.f, 1.f);
            BruteforceSearch<float> idx(space, n + 8);
            std::vector<float> first(dim), r(dim);
            for (size_t i = 0; i < n; ++i) {
                for (auto &v : r) v = g(rng);
                if (i == 0) first = r;
                if (i % 7 == 3) r = first;                                   // exact duplicates: ties at every radius
                idx.addPoint(r.data(), (labeltype)(i < 900 ? 2 * i : 2 * (i - 900) + 1));   // the last rows interleave: a re-sort by label
            }
            std::vector<float> q(dim);
            for (auto &v : q) v = g(rng);
            const char *what = pass == 0 ? "L2 64-d" : "IP 37-d";
            if (!radii(idx, q.data(), 5, what) || !radii(idx, first.data(), 10, what)) return 1;
            for (int t = 0; t < 9; ++t) idx.removePoint((labeltype)(2 * (50 + 40 * t)));   // dropped on the device
            idx.removePoint(0);                                                           // the row every duplicate copies
            if (!radii(idx, q.data(), 6, what)) return 1;
        }
    }
    {   // the int space: 32 bytes (norms on the device) and 5 (single bytes, the tail byte dropped)
        for (int pass = 0; pass < 2; ++pass) {
            const size_t dim = pass == 0 ? 32 : 5;
            L2SpaceI space(dim);
            BruteforceSearch<int> idx(&space, n + 8);
            std::vector<unsigned char> first(dim), r(dim);
            for (size_t i = 0; i < n; ++i) {
                for (auto &v : r) v = (unsigned char)(rng() & 255);
                if (i == 0) first = r;
                if (i % 7 == 3) r = first;
                idx.addPoint(r.data(), (labeltype)(3 * i));
            }
            std::vector<unsigned char> q(dim);
            for (auto &v : q) v = (unsigned char)(rng() & 255);
            const char *what = pass == 0 ? "L2I 32-d" : "L2I 5-d";
            if (!radii(idx, q.data(), 5, what) || !radii(idx, first.data(), 10, what)) return 1;
            idx.removePoint(0);
            idx.removePoint(3 * 700);
            if (!radii(idx, q.data(), 6, what)) return 1;
        }
    }
    printf("OK\n");
    return 0;
}
