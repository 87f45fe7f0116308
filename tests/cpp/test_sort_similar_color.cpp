// test_sort_similar_color.cpp -- the -sort-similar drop-in of the colour index (GpuColorDescIndex::gpuSortSimilar,
// cbird_amd/cpp/gpu_indexes.h) compiled against the mock cbird headers, run on the MI355X and compared with the table
// model by the Python test (tests/test_sort_similar_table.py).
//
//   test_sort_similar_color <file> : int32 cases; per case int32 entries, items, then entries x (uint32 id, 258-byte
//   descriptor) for the index in add order and items x (uint32 id, 258-byte descriptor) for the selection in selection
//   order.  Prints per case "case c queries notFound : id id ...".
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "index.h"
#include "gpu_indexes.h"

static bool readMedia(FILE* f, int32_t count, MediaGroup* out) {
  static_assert(sizeof(ColorDescriptor) == 258, "the reference's record");
  for (int32_t i = 0; i < count; ++i) {
    uint32_t id;
    ColorDescriptor d;
    if (fread(&id, 4, 1, f) != 1 || fread(&d, sizeof d, 1, f) != 1) return false;
    Media m(QString("/db/" + std::to_string(id) + ".jpg"), int(id), 0);
    m.setColorDescriptor(d);
    out->append(m);
  }
  return true;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  int32_t cases = 0;
  if (!f || fread(&cases, 4, 1, f) != 1) return 2;
  for (int32_t c = 0; c < cases; ++c) {
    int32_t head[2];
    if (fread(head, 4, 2, f) != 2) return 2;
    MediaGroup entries, selection;
    if (!readMedia(f, head[0], &entries) || !readMedia(f, head[1], &selection)) return 2;
    GpuColorDescIndex index(0);
    index.add(entries);
    SearchParams params;
    params.algo = SearchParams::AlgoColor;
    int queries = -1, notFound = -1;
    if (!index.gpuSortSimilar(selection, params, &queries, &notFound)) return 3;
    printf("case %d %d %d :", c, queries, notFound);
    for (const Media& m : selection) printf(" %d", m.id());
    printf("\n");
  }
  fclose(f);
  // the path attributes have to be parallel to the selection: refused, the selection stays
  MediaGroup two;
  ColorDescriptor d;
  d.numColors = 1;
  for (int id = 1; id <= 2; ++id) {
    Media m(QString("/db/" + std::to_string(id) + "/x.jpg"), id, 0);
    d.colors[0].l = uint16_t(1000 * id);
    m.setColorDescriptor(d);
    two.append(m);
  }
  GpuColorDescIndex index(0);
  index.add(two);
  GpuColorDescIndex::SortSimilarPaths paths;
  paths.filterParent = true;
  int q = 0, nf = 0;
  SearchParams params;
  params.algo = SearchParams::AlgoColor;
  if (index.gpuSortSimilar(two, params, &q, &nf, &paths) || two.count() != 2) return 4;
  paths.dirId = {0, 1};
  if (!index.gpuSortSimilar(two, params, &q, &nf, &paths) || two.count() != 2 || q != 2 || nf != 1) return 5;
  return 0;
}
