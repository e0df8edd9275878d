// hnsw_search -- batched search over a graph saved by the reference's HierarchicalNSW::saveIndex.
//   hnsw_search <index file> <queries.bin> <dim> <k> <ef> <out.txt> [ip|l2] [--allow FILE]
// queries.bin: raw fp32 [nq][dim].  out.txt: one line per query, "label:dist" pairs in ascending (dist, label)
// order -- what makeSearch.cpp:49-60 reads off searchKnn, for a whole batch at once.
// --allow FILE: one label per line; only nodes with one of these labels may be results (searchKnn with a BaseFilterFunctor:
// cvtmi_hnsw_search_masked).  The graph is traversed as without it; a query may return fewer than k pairs.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <unordered_set>
#include <vector>

#include "../hnswlib/hnswlib.h"

static const char *kUsage = "usage: hnsw_search <index> <queries.bin> <dim> <k> <ef> <out.txt> [ip|l2] [--allow FILE]\n"
                            "  --allow FILE  one label per line: only nodes with these labels may be returned\n";

struct AllowSet : hnswlib::BaseFilterFunctor {
    std::unordered_set<hnswlib::labeltype> ok;
    bool operator()(hnswlib::labeltype l) { return ok.count(l) != 0; }
};

int main(int argc, char *argv[])
{
    // options may stand anywhere behind the six positional arguments; anything malformed is a usage error (exit status 2)
    const char *allow = NULL, *space_arg = NULL;
    bool bad = false;
    for (int i = 7; i < argc; ++i) {
        if (!strcmp(argv[i], "--allow")) {
            if (allow || i + 1 >= argc) { bad = true; break; }
            allow = argv[++i];
        } else if (!strncmp(argv[i], "--", 2) || space_arg) {
            bad = true; break;
        } else {
            space_arg = argv[i];
        }
    }
    if (argc >= 7 && bad) {
        std::cerr << kUsage;
        return 2;
    }
    if (argc < 7) {
        std::cout << kUsage;
        return -1;
    }
    const int dim = atoi(argv[3]), k = atoi(argv[4]), ef = atoi(argv[5]);
    const bool l2 = space_arg && !strcmp(space_arg, "l2");
    std::ifstream in(argv[2], std::ios::binary | std::ios::ate);
    if (!in) { std::cout << "cannot open " << argv[2] << "\n"; return 1; }
    const size_t bytes = (size_t)in.tellg();
    in.seekg(0);
    const size_t nq = bytes / (sizeof(float) * (size_t)dim);
    std::vector<float> q(nq * (size_t)dim);
    in.read((char *)q.data(), (std::streamsize)(nq * dim * sizeof(float)));
    AllowSet filter;
    if (allow) {
        std::ifstream af(allow);
        if (!af) { std::cout << "cannot open " << allow << "\n"; return 1; }
        unsigned long long v;
        while (af >> v) filter.ok.insert((hnswlib::labeltype)v);
        if (!af.eof()) { std::cout << allow << ": not a list of labels\n"; return 1; }
    }
    try {
        hnswlib::InnerProductSpace ip((size_t)dim);
        hnswlib::L2Space l2s((size_t)dim);
        hnswlib::SpaceInterface<float> *space = l2 ? (hnswlib::SpaceInterface<float> *)&l2s : (hnswlib::SpaceInterface<float> *)&ip;
        hnswlib::HierarchicalNSW<float> alg(space, std::string(argv[1]));
        alg.setEf((size_t)ef);
        std::vector<std::priority_queue<std::pair<float, hnswlib::labeltype> > > res =
            alg.searchKnnBatch(q.data(), nq, (size_t)k, allow ? (hnswlib::BaseFilterFunctor *)&filter : (hnswlib::BaseFilterFunctor *)NULL);
        FILE *f = fopen(argv[6], "w");
        if (!f) { std::cout << "cannot write " << argv[6] << "\n"; return 1; }
        for (size_t i = 0; i < nq; ++i) {
            std::vector<std::pair<float, hnswlib::labeltype> > v;
            while (!res[i].empty()) { v.push_back(res[i].top()); res[i].pop(); }
            for (size_t j = v.size(); j-- > 0;) fprintf(f, "%zu:%.9g ", (size_t)v[j].second, (double)v[j].first);
            fprintf(f, "\n");
        }
        fclose(f);
        std::cout << nq << " queries over " << alg.ntotal() << " nodes" << std::endl;
    } catch (const std::exception &e) {
        std::cout << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
