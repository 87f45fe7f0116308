// test_clusters.cpp -- the clusters drop-in (GpuDctHashIndex::gpuClusters, cbird_amd/cpp/gpu_dcthashindex.h) compiled
// against the mock cbird headers, run on the MI355X and compared with the model by the Python test
// (tests/test_clusters_cpp.py).
//
//   test_clusters <file> : int32 cases; per case int32 n, thresh, minMatches, then n x (uint32 id, uint64 hash) in slot
//   order.  A fresh index is loaded with every item.  Prints "case c clusters" and per cluster "id:score id:score ...".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "index.h"
#include "gpu_dcthashindex.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t cases = 0;
  if (!f || fread(&cases, 4, 1, f) != 1) return 2;
  for (int32_t c = 0; c < cases; ++c) {
    int32_t head[3];
    if (fread(head, 4, 3, f) != 3) return 2;
    QSqlDatabase db;
    for (int32_t i = 0; i < head[0]; ++i) {
      uint32_t id;
      uint64_t hash;
      if (fread(&id, 4, 1, f) != 1 || fread(&hash, 8, 1, f) != 1) return 2;
      db.media.push_back({id, 1, int64_t(hash)});
    }
    GpuDctHashIndex index(0);
    index.load(db, "", "");
    SearchParams params;
    params.dctThresh = head[1];
    params.minMatches = head[2];
    const QVector<QVector<Index::Match>> groups = index.gpuClusters(params);
    printf("case %d %d\n", c, int(groups.size()));
    for (const QVector<Index::Match>& g : groups) {
      for (const Index::Match& m : g) printf("%u:%d ", m.mediaId, m.score);
      printf("\n");
    }
  }
  fclose(f);
  return 0;
}
