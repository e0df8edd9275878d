// opq_remove -- take videos out of an index file (IVFOPQ::RemoveVideos; the reference can only rebuild):
//   opq_remove <model> <index_file> <out_dir> <video_id>...
// The video ids are positions in the list the index was built from.  Writes the index IndexDatabase builds over the kept
// feature files alone, under the name SaveIndex gives it.
#include <cstdlib>
#include <iostream>
#include "../IVFOPQ.h"
using namespace std;
int main(int argc, char *argv[])
{
    if (argc < 5) {
        cerr << "usage: opq_remove <model> <index_file> <out_dir> <video_id>..." << endl;
        return 2;
    }
    string modelFile = argv[1], indexFile = argv[2], desDir = argv[3];
    vector<int> ids;
    for (int i = 4; i < argc; ++i) {
        char *end = NULL;
        long v = strtol(argv[i], &end, 10);
        if (end == argv[i] || *end) {
            cerr << "opq_remove: bad video id '" << argv[i] << "'" << endl;
            return 2;
        }
        ids.push_back((int)v);
    }
    IVFOPQ index;
    if (index.LoadModel(modelFile) != 1) return 1;
    index.LoadIndex(indexFile);
    const int before = index.numImages();
    const int removed = index.RemoveVideos(ids);
    if (removed < 0) {
        cerr << "opq_remove: " << index.lastError() << endl;
        return 1;
    }
    cout << "removed " << removed << " entries of " << before - index.numImages() << " videos, " << index.numImages() << " videos left" << endl;
    index.SaveIndex(desDir);
    return 0;
}
