// bf_remove_check -- self-check of hnswlib::BruteforceSearch::removePoint on the device (cvt_amd/host/hnswlib/bruteforce.h):
// once the rows are on the device, rounds of removePoint followed by a search drop the rows there (cvtmi_flat_remove_labels) and must
// answer exactly like an index built from scratch over the remaining rows -- without a full upload.  A round that mixes removals with
// ascending appends does not need one either; a label below one already uploaded does.  Prints "OK rebuilds=<n>" (n = full uploads
// after the first one) and returns 0, or the first difference.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../hnswlib/hnswlib.h"

using namespace hnswlib;

static bool same(BruteforceSearch<float> &a, const std::vector<float> &rows, const std::vector<labeltype> &labels, size_t dim,
                 SpaceInterface<float> *space, const std::vector<float> &q, size_t nq, size_t k, const char *what)
{
    BruteforceSearch<float> fresh(space, labels.size() + 1);
    for (size_t i = 0; i < labels.size(); ++i) fresh.addPoint((void *)&rows[i * dim], labels[i]);
    std::vector<float> d1(nq * k), d2(nq * k);
    std::vector<int64_t> l1(nq * k), l2(nq * k);
    a.searchKnnBatch(q.data(), nq, k, d1.data(), l1.data());
    fresh.searchKnnBatch(q.data(), nq, k, d2.data(), l2.data());
    for (size_t i = 0; i < nq * k; ++i)
        if (l1[i] != l2[i] || d1[i] != d2[i]) {
            printf("MISMATCH after %s: entry %zu: (%g, %lld) vs (%g, %lld)\n", what, i, d1[i], (long long)l1[i], d2[i], (long long)l2[i]);
            return false;
        }
    return true;
}

int main()
{
    const size_t dim = 64, nq = 7, k = 10;
    std::mt19937 rng(11);
    std::normal_distribution<float> g(0.f, 1.f);
    L2Space space(dim);
    BruteforceSearch<float> idx(&space, 5000);
    std::vector<float> rows;
    std::vector<labeltype> labels;
    std::vector<float> q(nq * dim);
    for (auto &v : q) v = g(rng);
    auto add = [&](labeltype lab) {
        std::vector<float> r(dim);
        for (auto &v : r) v = g(rng);
        if (lab % 7 == 0 && !rows.empty()) r.assign(rows.begin(), rows.begin() + dim);  // duplicates: (distance, label) ties
        idx.addPoint(r.data(), lab);
        rows.insert(rows.end(), r.begin(), r.end());
        labels.push_back(lab);
    };
    // removePoint moves the last row into the hole (brutoforce.hpp:58-70): mirror that in the expectation
    auto remove_at = [&](size_t victim) {
        idx.removePoint(labels[victim]);
        const size_t last = labels.size() - 1;
        labels[victim] = labels[last];
        for (size_t e = 0; e < dim; ++e) rows[victim * dim + e] = rows[last * dim + e];
        labels.pop_back();
        rows.resize(rows.size() - dim);
    };
    for (labeltype l = 0; l < 1000; ++l) add(l * 2);
    if (!same(idx, rows, labels, dim, &space, q, nq, k, "first 1000 rows")) return 1;   // the first upload
    const size_t base = idx.device_rebuilds;
    for (int round = 0; round < 4; ++round) {                                           // removals only: dropped on the device
        for (int t = 0; t < 5 + round; ++t) remove_at((size_t)(rng() % labels.size()));
        if (round == 1) remove_at(0);                                                   // the row every duplicate copies: ties change
        if (!same(idx, rows, labels, dim, &space, q, nq, k, "removePoint round")) return 1;
    }
    if (idx.device_rebuilds != base) { printf("MISMATCH: removal-only rounds rebuilt the device copy %zu times\n", idx.device_rebuilds - base); return 1; }
    // removals, then ascending appends (all rows were on the device when the removals came): still no rebuild
    for (int t = 0; t < 6; ++t) remove_at((size_t)(rng() % labels.size()));
    for (labeltype l = 3000; l < 3050; ++l) add(l);
    if (!same(idx, rows, labels, dim, &space, q, nq, k, "removals + ascending appends")) return 1;
    if (idx.device_rebuilds != base) { printf("MISMATCH: the mixed round rebuilt the device copy\n"); return 1; }
    // a removal, then a label below the largest uploaded one: a full re-sort
    remove_at((size_t)(rng() % labels.size()));
    add(4000);
    add(1001);
    if (!same(idx, rows, labels, dim, &space, q, nq, k, "removal + out-of-order label")) return 1;
    // and afterwards removals go to the device again
    for (int t = 0; t < 3; ++t) remove_at((size_t)(rng() % labels.size()));
    if (!same(idx, rows, labels, dim, &space, q, nq, k, "removePoint after re-sort")) return 1;
    printf("OK rebuilds=%zu\n", idx.device_rebuilds - base);
    return 0;
}
