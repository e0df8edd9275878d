// pca_train -- pca_train_project/train/src/train.cpp as a tool, its hard-coded values turned into arguments:
//   pca_train <feats.txt> <out.yml> [dim=2048] [num_reduced_dim=256]
// feats.txt: one row per line, "id,v1,...,vD" (what train.cpp and pca_project read); lines of another width are skipped
// and counted ("feat size != 2048" in the reference).  The model is trained on the MI355X (cvtk::PCAUtils::train ->
// cvtmi_pca_train) and written as OpenCV FileStorage YAML (PCAUtils::saveModel), the layout of the reference's models.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "../pca_utils.h"

int main(int argc, char *argv[])
{
    if (argc < 3) {
        std::cout << "usage: pca_train <feats.txt> <out.yml> [dim=2048] [num_reduced_dim=256]\n";
        return -1;
    }
    const int dim = argc > 3 ? atoi(argv[3]) : 2048;
    const int num_reduced_dim = argc > 4 ? atoi(argv[4]) : 256;
    if (dim < 1 || num_reduced_dim < 1) { std::cout << "bad dim / num_reduced_dim\n"; return -1; }
    try {
        std::ifstream fin(argv[1]);
        if (!fin) { std::cout << "cannot open " << argv[1] << "\n"; return 1; }
        std::vector<float> feats, row;
        std::string line;
        long rows = 0, skipped = 0;
        while (std::getline(fin, line)) {
            if (line.empty()) continue;
            const size_t comma = line.find(',');
            row.clear();
            if (comma != std::string::npos) {
                const char *c = line.c_str() + comma + 1;
                while (*c) {
                    char *next = NULL;
                    const float v = strtof(c, &next);  // std::stof in the reference (train.cpp:18)
                    if (next == c) break;
                    row.push_back(v);
                    c = (*next == ',') ? next + 1 : next;
                }
            }
            if ((int)row.size() != dim) { ++skipped; continue; }
            feats.insert(feats.end(), row.begin(), row.end());
            if (++rows % 10000 == 0) std::cout << "---> " << rows << std::endl;
        }
        if (skipped) std::cout << skipped << " lines skipped: feat size != " << dim << std::endl;
        if (rows > 0x7fffffffL) { std::cout << "too many rows\n"; return 1; }
        cvtk::PCAUtils &pca = *cvtk::PCAUtils::getInstance();
        pca.train(feats.data(), (int)rows, dim, num_reduced_dim);
        pca.saveModel(argv[2]);
        std::cout << rows << " rows trained " << dim << " -> " << num_reduced_dim << ", model written to " << argv[2] << std::endl;
    } catch (const std::exception &e) {
        std::cout << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
