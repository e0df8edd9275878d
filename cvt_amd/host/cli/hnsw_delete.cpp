// hnsw_delete -- mark nodes of a saved HierarchicalNSW graph deleted (current hnswlib's markDelete), or live again.
//   hnsw_delete <index in> <labels.txt> <index out> [--unmark]
// labels.txt: one label per line; every node that carries one of them changes state (duplicates and labels the graph does not
// hold are fine).  The output is the input with bit 16 of those nodes' level-0 count words set (cleared): the file hnswlib writes
// after markDelete.  hnsw_search never returns a marked node, hnsw_add links no new row to one.  No device is needed: the mark is
// made on the host image (loadIndex, markDeleteBatch, saveIndex).  The dimension is read from the file's header.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

#include "../hnswlib/hnswlib.h"

static int usage(std::ostream &o, int rc)
{
    o << "usage: hnsw_delete <index in> <labels.txt> <index out> [--unmark]\n"
         "  labels.txt  one label per line: the nodes that carry them are marked deleted (--unmark: live again)\n";
    return rc;
}

int main(int argc, char *argv[])
{
    if (argc < 4) return usage(std::cout, -1);
    if (argc > 5 || (argc == 5 && strcmp(argv[4], "--unmark"))) return usage(std::cerr, 2);
    const bool unmark = argc == 5;
    std::vector<hnswlib::labeltype> labels;
    {
        std::ifstream lf(argv[2]);
        if (!lf) { std::cout << "cannot open " << argv[2] << "\n"; return 1; }
        unsigned long long v;
        while (lf >> v) labels.push_back((hnswlib::labeltype)v);
        if (!lf.eof()) { std::cout << argv[2] << ": not a list of labels\n"; return 1; }
    }
    uint64_t head[6] = { 0, 0, 0, 0, 0, 0 };   // offsetLevel0, max_elements, cur_element_count, size_data_per_element, label_offset, offsetData
    {
        std::ifstream in(argv[1], std::ios::binary);
        if (!in || !in.read((char *)head, sizeof head)) { std::cout << "cannot read " << argv[1] << "\n"; return 1; }
    }
    if (head[4] <= head[5] || (head[4] - head[5]) % 4) { std::cout << argv[1] << ": not a saveIndex file\n"; return 1; }
    const size_t dim = (size_t)((head[4] - head[5]) / 4);
    try {
        hnswlib::InnerProductSpace space(dim);   // (marking computes no distance: either space reads the file)
        hnswlib::HierarchicalNSW<float> alg(&space, std::string(argv[1]));
        const size_t changed = unmark ? alg.unmarkDeleteBatch(labels.data(), labels.size()) : alg.markDeleteBatch(labels.data(), labels.size());
        alg.saveIndex(argv[3]);
        std::cout << changed << " nodes " << (unmark ? "unmarked" : "marked") << ", " << alg.deletedCount() << " of " << alg.ntotal()
                  << " deleted" << std::endl;
    } catch (const std::exception &e) {
        std::cout << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
