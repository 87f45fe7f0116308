// test_sort_similar.cpp -- the -sort-similar drop-in (GpuDctHashIndex::gpuSortSimilar, cbird_amd/cpp/gpu_dcthashindex.h)
// compiled against the mock cbird headers, run on the MI355X and compared with the issue's vectors by the Python test
// (tests/test_sort_similar.py).
//
//   test_sort_similar <file> : int32 cases; per case int32 n, thresh, then n x (uint32 id, uint64 hash) in selection
//   order.  A fresh index is loaded with every item.  Prints per case "case c queries notFound : id id ...".
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
    int32_t head[2];
    if (fread(head, 4, 2, f) != 2) return 2;
    MediaGroup selection;
    for (int32_t i = 0; i < head[0]; ++i) {
      uint32_t id;
      uint64_t hash;
      if (fread(&id, 4, 1, f) != 1 || fread(&hash, 8, 1, f) != 1) return 2;
      selection.append(Media(QString("/db/" + std::to_string(id) + ".jpg"), int(id), hash));
    }
    QSqlDatabase db;
    for (const Media& m : selection) db.media.push_back({uint32_t(m.id()), 1, int64_t(m.dctHash())});
    GpuDctHashIndex index(0);
    index.load(db, "", "");
    SearchParams params;
    params.dctThresh = head[1];
    int queries = -1, notFound = -1;
    if (!index.gpuSortSimilar(selection, params, &queries, &notFound)) return 3;
    printf("case %d %d %d :", c, queries, notFound);
    for (const Media& m : selection) printf(" %d", m.id());
    printf("\n");
  }
  fclose(f);
  // the path attributes have to be parallel to the selection: refused, the selection stays
  MediaGroup two;
  two.append(Media(QString("/db/a/1.jpg"), 1, 0xffull));
  two.append(Media(QString("/db/b/2.jpg"), 2, 0xfeull));
  QSqlDatabase db;
  for (const Media& m : two) db.media.push_back({uint32_t(m.id()), 1, int64_t(m.dctHash())});
  GpuDctHashIndex index(0);
  index.load(db, "", "");
  GpuDctHashIndex::SortSimilarPaths paths;
  paths.filterParent = true;
  int q = 0, nf = 0;
  if (index.gpuSortSimilar(two, SearchParams(), &q, &nf, &paths) || two.count() != 2) return 4;
  paths.dirId = {0, 1};
  if (!index.gpuSortSimilar(two, SearchParams(), &q, &nf, &paths) || two.count() != 2 || q != 2 || nf != 1) return 5;
  return 0;
}
