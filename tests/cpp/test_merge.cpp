// test_merge.cpp -- the -merge drop-in (GpuDctHashIndex::gpuMerge, cbird_amd/cpp/gpu_dcthashindex.h) compiled against the
// mock cbird headers, run on the MI355X and compared with database.merge by the Python test (tests/test_merge.py).
//
//   test_merge <file> : int32 cases; per case int32 nA, nB, thresh, then nA + nB x (uint32 id, uint64 hash), A then B.
//   A fresh index is loaded with every item.  Prints per case "case c unanswered k k ... : id id ...".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "index.h"
#include "gpu_dcthashindex.h"

static Media item(uint32_t id, uint64_t hash) { return Media(QString("/db/" + std::to_string(id) + ".jpg"), int(id), hash); }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t cases = 0;
  if (!f || fread(&cases, 4, 1, f) != 1) return 2;
  for (int32_t c = 0; c < cases; ++c) {
    int32_t head[3];
    if (fread(head, 4, 3, f) != 3) return 2;
    MediaGroup setA, setB;
    for (int32_t i = 0; i < head[0] + head[1]; ++i) {
      uint32_t id;
      uint64_t hash;
      if (fread(&id, 4, 1, f) != 1 || fread(&hash, 8, 1, f) != 1) return 2;
      (i < head[0] ? setA : setB).append(item(id, hash));
    }
    QSqlDatabase db;
    for (const MediaGroup* g : {&setA, &setB})
      for (const Media& m : *g) db.media.push_back({uint32_t(m.id()), 1, int64_t(m.dctHash())});
    GpuDctHashIndex index(0);
    index.load(db, "", "");
    SearchParams params;
    params.dctThresh = head[2];
    QVector<int> unanswered;
    if (!index.gpuMerge(setA, setB, params, &unanswered)) return 3;
    printf("case %d unanswered", c);
    for (int k : unanswered) printf(" %d", k);
    printf(" :");
    for (const Media& m : setA) printf(" %d", m.id());
    printf("\n");
  }
  fclose(f);
  // the two halves: a match the caller's own cascade supplies for an unanswered needle is placed like any other
  MediaGroup a, b;
  a.append(item(1, 0xffull));
  a.append(item(2, 0xff00ull));
  b.append(item(3, 0xfeull));
  b.append(item(4, 0xf0f0f0f0ull));
  QSqlDatabase db;
  for (const MediaGroup* g : {&a, &b})
    for (const Media& m : *g) db.media.push_back({uint32_t(m.id()), 1, int64_t(m.dctHash())});
  GpuDctHashIndex index(0);
  index.load(db, "", "");
  std::vector<uint32_t> match;
  std::vector<int32_t> score;
  if (!index.gpuMergeFind(a, b, SearchParams(), &match, &score)) return 4;
  if (match != std::vector<uint32_t>{0u, 0xffffffffu} || score != std::vector<int32_t>{1, -1}) return 5;
  match[1] = 2;  // "the colour stage" answers with the first needle
  std::vector<uint8_t> status;
  MediaGroup merged = a;
  if (!GpuDctHashIndex::mergePlace(merged, b, match, &status)) return 6;
  if (merged.count() != 4 || merged[0].id() != 4 || merged[1].id() != 3 || merged[2].id() != 1 || merged[3].id() != 2)
    return 7;
  if (status != std::vector<uint8_t>{CBH_MERGE_PLACED, CBH_MERGE_PLACED}) return 8;
  // the path attributes have to be parallel to A then B: refused, A stays
  GpuDctHashIndex::SortSimilarPaths paths;
  paths.filterParent = true;
  QVector<int> open;
  if (index.gpuMerge(a, b, SearchParams(), &open, &paths) || a.count() != 2) return 9;
  paths.dirId = {0, 1, 0, 1};  // needle 3 shares its directory with its only match
  if (!index.gpuMerge(a, b, SearchParams(), &open, &paths) || a.count() != 2 || open.count() != 2) return 10;
  return 0;
}
