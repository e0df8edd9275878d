// hnsw_add -- grow a saved HierarchicalNSW graph the way hnswlib is used for it: HierarchicalNSW(space, location), one addPoint per
// new row, saveIndex.
//   hnsw_add <index in> <rows.bin> <dim> <index out> [ip|l2] [labels.bin|-] [host|gpu|gpu:<max_batch>] [cont]
// rows.bin: raw fp32 [m][dim]; labels.bin: raw uint64 [m] (default / "-": the internal id, count + row).  The capacity becomes
// max(max_elements, count + m) (resizeIndex).  host (default): the addPoint loop, the file the reference writes from the same index
// and rows.  gpu / gpu:<max_batch>: cvtmi_hnsw_add on the device copy (addPointsGpu; gpu:1 is the sequential algorithm and writes
// the same file as host; gpu = the default schedule).
// Levels: loadIndex leaves the level generator at its initialiser, in the reference and here, so the added rows get the draws a
// fresh build gives its first m rows.  cont puts the stream at cur_element_count draws first: the result continues the build that
// wrote the index (hnsw_build of n0 rows + hnsw_add ... cont of the rest = hnsw_build of all rows).
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "../hnswlib/hnswlib.h"

template <typename T> static bool slurp(const char *path, std::vector<T> &v)
{
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) return false;
    const size_t bytes = (size_t)in.tellg();
    in.seekg(0);
    v.resize(bytes / sizeof(T));
    in.read((char *)v.data(), (std::streamsize)(v.size() * sizeof(T)));
    return true;
}

static int usage(std::ostream &o, int rc)
{
    o << "usage: hnsw_add <index in> <rows.bin> <dim> <index out> [ip|l2] [labels.bin|-] [host|gpu|gpu:<max_batch>] [cont]\n";
    return rc;
}

int main(int argc, char *argv[])
{
    if (argc < 5) return usage(std::cout, -1);
    if (argc > 9) return usage(std::cerr, 2);
    const size_t dim = (size_t)atoi(argv[3]);
    if (dim < 1) return usage(std::cerr, 2);
    const bool l2 = argc > 5 && !strcmp(argv[5], "l2");
    if (argc > 5 && !l2 && strcmp(argv[5], "ip")) return usage(std::cerr, 2);
    const char *mode = argc > 7 ? argv[7] : "host";
    const bool gpu = !strncmp(mode, "gpu", 3) && (mode[3] == '\0' || mode[3] == ':');
    if (!gpu && strcmp(mode, "host")) return usage(std::cerr, 2);
    const int max_batch = gpu && mode[3] == ':' ? atoi(mode + 4) : 0;
    if (max_batch < 0) return usage(std::cerr, 2);
    if (argc > 8 && strcmp(argv[8], "cont")) return usage(std::cerr, 2);
    const bool cont = argc > 8;
    std::vector<float> rows;
    std::vector<uint64_t> labels;
    if (!slurp(argv[2], rows)) { std::cout << "cannot open " << argv[2] << "\n"; return 1; }
    if (argc > 6 && strcmp(argv[6], "-") && !slurp(argv[6], labels)) { std::cout << "cannot open " << argv[6] << "\n"; return 1; }
    const size_t m = rows.size() / dim;
    if (!labels.empty() && labels.size() != m) { std::cout << "labels.bin does not hold one label per row\n"; return 1; }
    try {
        hnswlib::InnerProductSpace ip(dim);
        hnswlib::L2Space l2s(dim);
        hnswlib::SpaceInterface<float> *space = l2 ? (hnswlib::SpaceInterface<float> *)&l2s : (hnswlib::SpaceInterface<float> *)&ip;
        hnswlib::HierarchicalNSW<float> alg(space, std::string(argv[1]));
        const size_t n0 = alg.ntotal();
        alg.resizeIndex(std::max(alg.maxElements(), n0 + m));
        if (cont) alg.setLevelDraws(n0);
        const auto t0 = std::chrono::steady_clock::now();
        if (gpu) {
            std::vector<hnswlib::labeltype> lab(labels.begin(), labels.end());
            alg.addPointsGpu(rows.data(), lab.empty() ? NULL : lab.data(), m, max_batch);
        } else {
            for (size_t i = 0; i < m; ++i)
                alg.addPoint(&rows[i * dim], labels.empty() ? (hnswlib::labeltype)(n0 + i) : (hnswlib::labeltype)labels[i]);
        }
        const auto t1 = std::chrono::steady_clock::now();
        alg.saveIndex(argv[4]);
        std::cout << m << " rows added to " << n0 << " (insert " << std::chrono::duration<double>(t1 - t0).count() << " s)" << std::endl;
    } catch (const std::exception &e) {
        std::cout << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
