// gpu_dcthashindex.h -- cbird-side binding of the MI355X DctHashIndex (drop-in for
// src/dcthashindex.{h,cpp}).
//
// This is the file a cbird maintainer adds to src/ (see INTEGRATION.md): a subclass of the
// reference's `Index` plugin interface (src/index.h:150-281) with exactly the overrides of
// DctHashIndex (src/dcthashindex.h:29-67).  All array work -- storage, add/remove, find, slice --
// goes through the C-ABI of libcbird_hip.so (include/cbird_hip.h); the SQL of load()/mediaIds()
// stays here, verbatim in meaning (`select id,phash_dct from media where type=1`,
// src/dcthashindex.cpp:82-89).
//
// It compiles against the real cbird headers ("index.h", Qt6) and, for this repository's tests
// where Qt6/OpenCV are not installed, against tests/cpp/mock/index.h which declares the same
// names with the same signatures.
#pragma once

#include <algorithm>
#include <string>
#include <vector>

#include "cbird_hip.h"
#include "gpu_devices.h"
#include "index.h"  // cbird's src/index.h (or the test mock)
#include "gpu_errors.h"

class GpuDctHashIndex : public Index {
  Q_DISABLE_COPY_MOVE(GpuDctHashIndex)

 public:
  explicit GpuDctHashIndex(int device = 0) : _device(device) {
    _id = SearchParams::AlgoDCT;  // dcthashindex.cpp:31
    _idx = cbh_idx64_create(device);
    if (!_idx) qFatal("GpuDctHashIndex: no usable MI355X (gfx950) device %d", device);
  }
  /// one index over several GPUs: `new GpuDctHashIndex(GpuDeviceSet::all())` in Engine::Engine
  explicit GpuDctHashIndex(const GpuDeviceSet& devs) : _device(devs.first()) {
    _id = SearchParams::AlgoDCT;
    _idx = devs.single() ? cbh_idx64_create(_device) : cbh_idx64_create_sharded(devs.mask, devs.shardsPerDevice);
    if (!_idx) qFatal("GpuDctHashIndex: device mask 0x%x names a device that is not a usable MI355X", devs.mask);
  }
  ~GpuDctHashIndex() override { cbh_idx64_destroy(_idx); }

  bool isLoaded() const override { return cbh_idx64_is_loaded(_idx) != 0; }
  int count() const override { return int(cbh_idx64_count(_idx)); }
  size_t memoryUsage() const override { return cbh_idx64_memory_usage(_idx); }

  // DctHashIndex::load (dcthashindex.cpp:70-114): hashes always come from the database
  void load(QSqlDatabase& db, const QString& cachePath, const QString& dataPath) override {
    (void)cachePath;
    (void)dataPath;
    if (isLoaded()) return;
    QSqlQuery query(db);
    query.setForwardOnly(true);
    if (!query.exec("select id,phash_dct from media where type=1")) SQL_FATAL(exec);
    std::vector<uint64_t> hashes;
    std::vector<uint32_t> ids;
    while (query.next()) {
      ids.push_back(query.value(0).toUInt());
      hashes.push_back(uint64_t(query.value(1).toLongLong()));
    }
    mutate("load", [&] { return cbh_idx64_load(_idx, hashes.data(), ids.data(), hashes.size()); });
  }

  void save(QSqlDatabase& db, const QString& cachePath) override {
    (void)db;
    (void)cachePath;  // nothing to cache: the SoA is rebuilt from SQL (dcthashindex.cpp:116-120)
  }

  QSet<mediaid_t> mediaIds(QSqlDatabase& db, const QString& cachePath,
                           const QString& dataPath) const override {
    (void)cachePath;
    (void)dataPath;
    QSet<mediaid_t> set;
    if (isLoaded()) {  // dcthashindex.cpp:129-133
      size_t n = 0;
      if (!query("mediaIds", [&] { return cbh_idx64_media_ids(_idx, nullptr, 0, &n); })) return set;
      std::vector<uint32_t> ids(n ? n : 1);
      if (!query("mediaIds", [&] { return cbh_idx64_media_ids(_idx, ids.data(), ids.size(), &n); })) return set;
      for (size_t i = 0; i < n; ++i) set.insert(ids[i]);
      return set;
    }
    QSqlQuery query(db);  // dcthashindex.cpp:136-153
    query.setForwardOnly(true);
    if (!query.exec("select id,phash_dct from media where type=1")) SQL_FATAL(exec);
    while (query.next()) {
      mediaid_t id = query.value(0).toUInt();
      uint64_t hash = uint64_t(query.value(1).toLongLong());
      if (hash != 0) set.insert(id);
    }
    return set;
  }

  // dcthashindex.cpp:158-173 (the tree rebuild disappears: the scan needs no tree)
  void add(const MediaGroup& media) override {
    std::vector<uint64_t> hashes;
    std::vector<uint32_t> ids;
    for (const Media& m : media) {
      hashes.push_back(m.dctHash());
      ids.push_back(uint32_t(m.id()));
    }
    mutate("add", [&] { return cbh_idx64_add(_idx, hashes.data(), ids.data(), hashes.size()); });
  }

  // dcthashindex.cpp:175-191
  void remove(const QVector<int>& removed) override {
    if (!isLoaded()) return;
    std::vector<uint32_t> ids;
    for (int id : removed) ids.push_back(uint32_t(id));
    mutate("remove", [&] { return cbh_idx64_remove(_idx, ids.data(), ids.size()); });
  }

  // dcthashindex.cpp:193-220.  Thread-safe for concurrent callers (QtConcurrent workers under
  // Database's read lock, database.cpp:1400-1432,1698).
  QVector<Index::Match> find(const Media& m, const SearchParams& p) override {
    QVector<Index::Match> results;
    uint64_t target = m.dctHash();
    if (!target) {
      qWarning() << "no hash for needle:" << m.path();
      return results;
    }
    if (count() <= 0) {
      qWarning() << "empty/null tree";
      return results;
    }
    // cbh_idx64_find_coalesced: same results as cbh_idx64_find; concurrent QtConcurrent workers share one scan per
    // round trip, and an all-pairs run (Database::similar) ends up served from one whole-index self-join
    std::vector<cbh_match> buf(64);
    size_t n = 0;
    for (;;) {
      if (!query("find", [&] { return cbh_idx64_find_coalesced(_idx, target, p.dctThresh, buf.data(), buf.size(), &n); }))
        return results;
      if (n <= buf.size()) break;
      buf.resize(n);
    }
    for (size_t i = 0; i < n; ++i) results.append(Index::Match(buf[i].id, buf[i].score));
    return results;
  }

  // dcthashindex.cpp:222-250; caller deletes (database.cpp:1435,1491)
  Index* slice(const QSet<uint32_t>& mediaIds) const override {
    Q_ASSERT(isLoaded());
    std::vector<uint32_t> ids;
    for (uint32_t id : mediaIds) ids.push_back(id);
    cbh_idx64* sub = cbh_idx64_slice(_idx, ids.data(), ids.size());
    if (!sub && cbh_last_error_code() == CBH_E_NOMEM) {  // transient: give cached scratch back, once more
      gpuidx::releaseScratch(cbh_idx64_device_mask(_idx));
      sub = cbh_idx64_slice(_idx, ids.data(), ids.size());
    }
    if (!sub) {  // a slice that cannot be made is an empty one (its searches find nothing), not the end of the process
      qCritical("GpuDctHashIndex::slice: %s", cbh_last_error());
      return new GpuDctHashIndex(_device);
    }
    return new GpuDctHashIndex(_device, sub);
  }

  /// MI355X-native extension used by a batched Database::similar: every needle of `needles` in
  /// one launch; results[i] = matches of needles[i] already sorted by (score, id) and cut at
  /// maxMatches+1 (room for the self match that searchIndex filters, database.cpp:1733-1735).
  QVector<QVector<Index::Match>> findBatch(const MediaGroup& needles, const SearchParams& p) {
    const int k = p.maxMatches + 1;
    std::vector<uint64_t> q;
    for (const Media& m : needles) q.push_back(m.dctHash());
    std::vector<cbh_match> out(q.size() * size_t(k));
    std::vector<uint32_t> counts(q.size());
    QVector<QVector<Index::Match>> res;
    if (!query("find_batch",
               [&] { return cbh_idx64_find_batch(_idx, q.data(), q.size(), p.dctThresh, k, out.data(), counts.data()); })) {
      for (size_t i = 0; i < q.size(); ++i) res.append(QVector<Index::Match>());
      return res;
    }
    for (size_t i = 0; i < q.size(); ++i) {
      QVector<Index::Match> r;
      const size_t m = std::min<size_t>(counts[i], size_t(k));
      for (size_t j = 0; j < m; ++j) r.append(Index::Match(out[i * k + j].id, out[i * k + j].score));
      res.append(r);
    }
    return res;
  }

  /// Database::searchIndex (src/database.cpp:1691-1757) for every needle in one call: the maxThresh escalation
  /// (only needles still at <= minMatches are searched again), (score, mediaId) order, filterSelf, the maxMatches cut,
  /// and ids that are not in `knownIds` (the caller's idMap keys, ascending; nullptr = all known) skipped WITHOUT
  /// consuming a place -- unlike findBatch above, whose fixed cut at maxMatches + 1 is only right when every index
  /// entry is a known media.  result[i] = the matches of needles[i] as searchIndex would append them to its group.
  QVector<QVector<Index::Match>> searchIndexBatch(const MediaGroup& needles, const SearchParams& p,
                                                  const std::vector<uint32_t>* knownIds = nullptr) {
    std::vector<uint64_t> q;
    std::vector<uint32_t> ids;
    for (const Media& m : needles) {
      q.push_back(m.dctHash());
      ids.push_back(uint32_t(m.id()));
    }
    const size_t k = size_t(p.maxMatches);
    std::vector<cbh_match> out(q.size() * std::max<size_t>(k, 1));
    std::vector<uint32_t> counts(q.size());
    QVector<QVector<Index::Match>> res;
    if (!query("search_index_batch", [&] {
          return cbh_search_index_batch(_idx, q.data(), ids.data(), q.size(), p.dctThresh, p.maxThresh, p.minMatches,
                                        p.maxMatches, p.filterSelf ? 1 : 0, knownIds ? knownIds->data() : nullptr,
                                        knownIds ? knownIds->size() : 0, out.data(), counts.data());
        })) {
      for (size_t i = 0; i < q.size(); ++i) res.append(QVector<Index::Match>());
      return res;
    }
    for (size_t i = 0; i < q.size(); ++i) {
      QVector<Index::Match> r;
      for (size_t j = 0; j < counts[i]; ++j) r.append(Index::Match(out[i * k + j].id, out[i * k + j].score));
      res.append(r);
    }
    return res;
  }

  /// What filterMatch reads from paths (src/database.cpp:1217-1242), parallel to the selection, for gpuSortSimilar:
  /// dirId[i] -- equal numbers <=> equal Media::dirPath() -- when params.filterParent, underPrefix[i] =
  /// path().startsWith(prefix) when params.path is set (pathMode 1 = inPath, 2 = not inPath).  INTEGRATION.md fills it.
  struct SortSimilarPaths {
    bool filterParent = false;
    int pathMode = 0;
    std::vector<uint32_t> dirId;
    std::vector<uint8_t> underPrefix;
  };
  /// `-sort-similar` (src/main.cpp:1523-1580) in one kernel launch instead of up to 5 (n - 1) slices and queries:
  /// `selection` becomes the sorted list (items never reached are dropped, :1579), *queries / *notFound count what the
  /// reference's loop counts.  AlgoDCT with mirrorMask 0 and no templateMatch; items this index does not hold are never
  /// candidates, as in the reference's slice.  false (selection untouched, the error logged): the call failed or the
  /// selection has more than CBH_SORT_SIMILAR_MAX items -- run the reference's loop then.
  bool gpuSortSimilar(MediaGroup& selection, const SearchParams& p, int* queries, int* notFound,
                      const SortSimilarPaths* paths = nullptr) const {
    const size_t n = selection.size();
    std::vector<uint64_t> hashes;
    std::vector<uint32_t> ids, order(n ? n : 1);
    for (const Media& m : selection) {
      hashes.push_back(m.dctHash());
      ids.push_back(uint32_t(m.id()));
    }
    std::vector<uint8_t> inIndex;
    if (!heldFlags(ids, &inIndex)) return false;
    cbh_sort_similar_params sp;
    sp.thresh = p.dctThresh, sp.max_thresh = p.maxThresh, sp.min_matches = p.minMatches, sp.max_matches = p.maxMatches;
    sp.filter_parent = paths && paths->filterParent, sp.path_mode = paths ? paths->pathMode : 0;
    sp.look_behind = 5;  // `const int lookBehind = 5` (:1530)
    if ((sp.filter_parent && paths->dirId.size() != n) || (sp.path_mode && paths->underPrefix.size() != n)) {
      qCritical("GpuDctHashIndex::gpuSortSimilar: the path attributes are not parallel to the selection");
      return false;
    }
    const uint64_t first[2] = {0, n};
    cbh_sort_similar_result res = {0, 0, 0, 0};
    if (!query("sort_similar", [&] {
          return cbh_sort_similar(hashes.data(), ids.data(), inIndex.data(), sp.filter_parent ? paths->dirId.data() : nullptr,
                                  sp.path_mode ? paths->underPrefix.data() : nullptr, first, 1, &sp, order.data(), &res,
                                  _device);
        }))
      return false;
    std::vector<std::pair<uint32_t, size_t>> where;  // id -> place in the selection
    for (size_t i = 0; i < n; ++i) where.push_back({ids[i], i});
    std::sort(where.begin(), where.end());
    MediaGroup sorted;
    for (uint32_t k = 0; k < res.sorted; ++k)
      sorted.append(selection[std::lower_bound(where.begin(), where.end(), std::make_pair(order[k], size_t(0)))->second]);
    selection = sorted;
    if (queries) *queries = int(res.queries);
    if (notFound) *notFound = int(res.not_found);
    return true;
  }

  /// The AlgoDCT stage of `-merge A B` (src/main.cpp:1582-1652) for every needle of B in one kernel launch instead of one
  /// slice and one query per needle: needle b_k is searched inside setA followed by b_0 .. b_k (:1619-1625) with
  /// multiSearch's maxMatches = 2 (:1591).  (*match)[k] = the place of its matches[0] in setA + setB (setA.size() + j for
  /// b_j), 0xFFFFFFFF without one; (*score)[k] = its distance, -1 without one.  `paths` is parallel to setA then setB.
  /// Items this index does not hold are never candidates, as in the reference's slice.  false (the error logged): the
  /// call failed.
  bool gpuMergeFind(const MediaGroup& setA, const MediaGroup& setB, const SearchParams& p, std::vector<uint32_t>* match,
                    std::vector<int32_t>* score, const SortSimilarPaths* paths = nullptr) const {
    const size_t nA = setA.size(), nB = setB.size(), n = nA + nB;
    std::vector<uint64_t> hashes;
    std::vector<uint32_t> ids;
    for (const MediaGroup* g : {&setA, &setB})
      for (const Media& m : *g) {
        hashes.push_back(m.dctHash());
        ids.push_back(uint32_t(m.id()));
      }
    std::vector<uint8_t> inIndex;
    if (!heldFlags(ids, &inIndex)) return false;
    cbh_merge_params mp;
    mp.thresh = p.dctThresh, mp.max_thresh = p.maxThresh, mp.min_matches = p.minMatches;
    mp.max_matches = 2;  // `search.params.maxMatches = 2` (:1591)
    mp.filter_parent = paths && paths->filterParent, mp.path_mode = paths ? paths->pathMode : 0;
    if ((mp.filter_parent && paths->dirId.size() != n) || (mp.path_mode && paths->underPrefix.size() != n)) {
      qCritical("GpuDctHashIndex::gpuMergeFind: the path attributes are not parallel to A then B");
      return false;
    }
    match->assign(nB ? nB : 1, 0xffffffffu);
    score->assign(nB ? nB : 1, -1);
    const bool ok = query("merge_find", [&] {
      return cbh_merge_find(hashes.data(), ids.data(), inIndex.data(), mp.filter_parent ? paths->dirId.data() : nullptr,
                            mp.path_mode ? paths->underPrefix.data() : nullptr, nA, nB, &mp, match->data(), score->data(),
                            _device);
    });
    match->resize(nB);
    score->resize(nB);
    return ok;
  }
  /// The placement of `-merge` (:1628-1650) for match[k] as gpuMergeFind writes it, from whichever stage of the cascade
  /// answered: setA becomes the merged list.  (*status)[k] (may be NULL) = CBH_MERGE_PLACED, CBH_MERGE_NO_MATCH ("no
  /// match", the needle is dropped) or CBH_MERGE_MATCH_UNPLACED (its match is a needle that was dropped: the reference's
  /// Q_ASSERT at :1640; here the needle is dropped too).  false (setA untouched, the error logged): a match outside A, B.
  static bool mergePlace(MediaGroup& setA, const MediaGroup& setB, const std::vector<uint32_t>& match,
                         std::vector<uint8_t>* status = nullptr) {
    const size_t nA = setA.size(), nB = setB.size();
    std::vector<uint64_t> hashes;
    for (const MediaGroup* g : {static_cast<const MediaGroup*>(&setA), &setB})
      for (const Media& m : *g) hashes.push_back(m.dctHash());
    std::vector<uint32_t> order(nA + nB + 1);
    std::vector<uint8_t> st(nB + 1);
    size_t len = 0;
    if (match.size() != nB ||
        cbh_merge_place(hashes.data(), nA, nB, match.data(), order.data(), st.data(), &len) != CBH_OK) {
      qCritical("GpuDctHashIndex::mergePlace: one match per needle, each a place in A then B");
      return false;
    }
    MediaGroup merged;
    for (size_t k = 0; k < len; ++k) merged.append(order[k] < nA ? setA[order[k]] : setB[order[k] - nA]);
    setA = merged;
    st.resize(nB);
    if (status) *status = st;
    return true;
  }
  /// `-merge` with AlgoDCT: gpuMergeFind, then mergePlace with every needle the stage answered at a score under 12
  /// (multiSearch's threshold for algo 0, :1594-1607).  *unanswered = the needles of setB, in B's order, that it did not
  /// answer so -- they are NOT placed: the caller's own cascade (fdct, ORB, colour through Engine::query) still has to try
  /// them before placing them.  The result is the reference's whenever *unanswered comes back empty; a caller that wants
  /// it for the other needles too completes `match` itself between the two halves, because a place
  /// depends on what was placed before.  false (setA untouched, the error logged): the call failed.
  bool gpuMerge(MediaGroup& setA, const MediaGroup& setB, const SearchParams& p, QVector<int>* unanswered,
                const SortSimilarPaths* paths = nullptr) const {
    std::vector<uint32_t> match;
    std::vector<int32_t> score;
    if (!gpuMergeFind(setA, setB, p, &match, &score, paths)) return false;
    QVector<int> open;
    for (size_t k = 0; k < match.size(); ++k)
      if (match[k] == 0xffffffffu || score[k] >= 12) {
        match[k] = 0xffffffffu;
        open.append(int(k));
      }
    if (!mergePlace(setA, setB, match)) return false;
    if (unanswered) *unanswered = open;
    return true;
  }

  /// The partition `-similar` cannot give: every connected component of this index's match graph at p.dctThresh with more
  /// than p.minMatches members (filterMatch's rule, src/database.cpp:1244; never fewer than two), as Match(mediaId, distance
  /// to the nearest other member) -- members in ascending id, clusters in ascending first id (cbh_idx64_clusters).  One
  /// device pass over the edges; Media::mergeGroupList on -similar's groups is neither transitive nor better than
  /// quadratic.  The caller maps the ids to Media and orders by path.  Empty (the error logged): the call
  /// failed, or nothing clusters.
  QVector<QVector<Index::Match>> gpuClusters(const SearchParams& p) const {
    QVector<QVector<Index::Match>> res;
    std::vector<uint64_t> first(1);
    std::vector<cbh_match> members(1);
    size_t nc = 0, nm = 0;
    if (!query("clusters", [&] {
          const int minMembers = std::max(2, p.minMatches + 1);
          int rc = cbh_idx64_clusters(_idx, p.dctThresh, minMembers, first.data(), first.size() - 1, members.data(),
                                      members.size(), &nc, &nm, nullptr);
          if (rc == CBH_E_OVERFLOW && (nc > first.size() - 1 || nm > members.size())) {  // the room needed: once more
            first.resize(nc + 1);
            members.resize(std::max<size_t>(nm, 1));
            rc = cbh_idx64_clusters(_idx, p.dctThresh, minMembers, first.data(), nc, members.data(), members.size(), &nc, &nm,
                                    nullptr);
          }
          return rc;
        }))
      return res;
    for (size_t g = 0; g < nc; ++g) {
      QVector<Index::Match> group;
      for (uint64_t t = first[g]; t < first[g + 1]; ++t) group.append(Index::Match(members[t].id, members[t].score));
      res.append(group);
    }
    return res;
  }

  cbh_idx64* handle() const { return _idx; }  // for statistics (cbh_idx64_get_stats / cbh_idx64_coalesce_stats)

 private:
  GpuDctHashIndex(int device, cbh_idx64* adopted) : _device(device), _idx(adopted) {
    _id = SearchParams::AlgoDCT;
  }
  // the reference has no error codes on this surface (gpu_errors.h, gpuidx::run): load/add/remove retry once after
  // releasing cached scratch and then abort like the reference's failed allocation; find & co. log and return nothing
  template <class Call>
  void mutate(const char* what, Call&& call) const {
    (void)gpuidx::run(gpuidx::Mutation, (std::string("GpuDctHashIndex::") + what).c_str(), call, cbh_idx64_device_mask(_idx));
  }
  template <class Call>
  bool query(const char* what, Call&& call) const {
    return gpuidx::run(gpuidx::Query, (std::string("GpuDctHashIndex::") + what).c_str(), call, cbh_idx64_device_mask(_idx));
  }
  // (*inIndex)[i] = a slice of this index can hold ids[i]: every entry with an id, a hash of 0 included (mediaIds()
  // leaves those out)
  bool heldFlags(const std::vector<uint32_t>& ids, std::vector<uint8_t>* inIndex) const {
    std::vector<uint32_t> held(cbh_idx64_count(_idx) ? cbh_idx64_count(_idx) : 1);
    std::vector<uint64_t> heldHashes(held.size());
    if (cbh_idx64_count(_idx) &&
        !query("download", [&] { return cbh_idx64_download(_idx, heldHashes.data(), held.data(), cbh_idx64_count(_idx)); }))
      return false;
    held.resize(cbh_idx64_count(_idx));
    std::sort(held.begin(), held.end());
    for (uint32_t id : ids) inIndex->push_back(id && std::binary_search(held.begin(), held.end(), id) ? 1 : 0);
    return true;
  }
  int _device;
  cbh_idx64* _idx;
};
