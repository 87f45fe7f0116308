// pipeline.hip -- Scanner::processImage (src/scanner.cpp:828-895) for a batch of decoded images of one geometry: the
// caller of every feature stage of the hot path, chained on the device.  One upload per chunk; between the stages only
// the autocrop rectangles (to pick launch geometries) and the keypoints (12 bytes each, to build the keypoint-hash work
// list) visit the host.  The stages of a chunk, each a function of IndexCall below:
//
//   gray            grayscale (or, with view_mask, k_gray_views / k_turn_views)   prestage, mirror, turns   (:859)
//   start_color     ColorDescriptor::create(cvColor), on a stream of its own      colordesc_create.hip      (:868-872)
//   kept_regions    autocrop(20), the launch plan of hash and resize              prestage.hip, cbh_regions.h
//   hash            dctHash64(view)                                               dcthash.hip               (:859-866)
//   resize          sizeLongestSide(cvGray, 400)                                  prestage.hip (Lanczos-4)  (:876)
//   orb             makeKeyPoints / makeKeyPointDescriptors, the keypoint lists   orb.hip                   (:878-884)
//   keypoint_hashes makeKeyPointHashes on the keypoints compute() left            kphash.hip (k_kp_hashes)  (:886-889)
// With view_mask (cbh_index_images_views[_ex]) the grey step writes the views of each uploaded image, and the stages after
// it run on those V planes per image: once on the w x h planes (identity and reflections) and once on the h x w planes
// (quarter turns and transposes), each pass writing its views' rows of the results.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "cbh_index.h"
#include "cbh_regions.h"
#include "cbh_staging.h"

namespace {

// the arguments of cbh_index_images_views_ex
struct IndexArgs {
  const uint8_t* imgs;
  size_t n;
  int w, h;
  size_t row_stride, img_stride;
  int channels, view_mask;
  const cbh_index_params* p;
  uint64_t* dct_hashes;
  int32_t *rects, *resized_dims;
  uint32_t* kp_counts;
  cbh_keypoint* kp;
  uint8_t* desc;
  uint32_t* kph_counts;
  uint64_t* kp_hashes;
  uint8_t *color_descs, *color_ok;
  int device;
};

// What a call owns besides its device blocks.  Each gives up its own on every way out of the call.
struct Stream {  // non-blocking; drained, then destroyed with its cached blocks handed on
  hipStream_t s = nullptr;
  hipError_t err;
  Stream() : err(hipStreamCreateWithFlags(&s, hipStreamNonBlocking)) {}
  Stream(const Stream&) = delete;
  ~Stream() {
    if (s) (void)hipStreamSynchronize(s), cbh::stream_destroy(s);
  }
};
struct Event {
  hipEvent_t ev = nullptr;
  hipError_t err;
  Event() : err(hipEventCreateWithFlags(&ev, hipEventDisableTiming)) {}
  Event(const Event&) = delete;
  ~Event() {
    if (ev) (void)hipEventDestroy(ev);
  }
};
struct Joined {
  std::thread t;
  void join() {
    if (t.joinable()) t.join();
  }
  ~Joined() { join(); }
};

// One index_images_one: what was asked for, the sizes, what the call owns, and the chunk in flight.
struct IndexCall {
  const IndexArgs& a;
  const cbh_index_params& p;
  const bool a_dct, a_fdct, a_orb, a_color, feats;
  const int rs, cap;
  size_t span1, per_chunk, V, Va, T, per_out, cview_off, tview_off, cview_bytes, tgray_off, slot;
  bool views, color_views;

  // Host state first, so that it leaves last: the colour thread reads coff / cw / chh / cst, and copies queued on s
  // write into cnt, hkp, hafter and hh -- all of them outlive the thread and both streams on every way out.
  std::vector<int> hr;  // the kept regions
  std::vector<cbh::RegionRun> plan;
  std::vector<size_t> base;
  std::vector<uint64_t> off, coff, hh, hd;
  std::vector<uint8_t> hdesc;
  std::vector<uint32_t> ws, hs, ow, oh, cw, chh, cst, cnt, kp_first, out_first;
  std::vector<cbh_keypoint> hkp;
  std::vector<float> hafter, tri;

  // the chunk in flight: images uploaded, its results and the index of their first; the pass in flight: its geometry,
  // its planes (vg views per image, the first of them view vfirst), their number
  size_t mu = 0, mt = 0, o0 = 0;
  const uint8_t *gray0 = nullptr, *gray = nullptr;
  size_t gs0 = 0, gi0 = 0, gs = 0, gi = 0, m = 0, vfirst = 0, vg = 1;
  int gw = 0, gh = 0;
  int color_rc = CBH_OK;

  // The owners leave in the reverse of this order, before anything declared above: the colour thread is joined, s2
  // drained and destroyed, the event destroyed, the blocks given back on s (to the cached pool, keep_pool_memory: the
  // next call reuses them), s drained and destroyed.  The colour kernels on s2 read blocks of s's cache, so s2 must be
  // drained before those go back.
  Stream s;
  cbh::Scratch blocks{s.s};
  Event ev_up;
  Stream s2;
  Joined color_thread;

  uint8_t *d_src = nullptr, *d_gray = nullptr, *d_res = nullptr, *d_desc = nullptr, *d_cdesc = nullptr, *d_cok = nullptr;
  uint64_t *d_out = nullptr, *d_kph = nullptr;
  int* d_rects = nullptr;
  cbh_keypoint* d_kp = nullptr;
  float* d_after = nullptr;
  uint32_t* d_cnt = nullptr;

  const bool trace = getenv("CBH_PIPELINE_TRACE") != nullptr;  // stage times of each chunk on stderr
  std::chrono::steady_clock::time_point t_last = std::chrono::steady_clock::now();

  explicit IndexCall(const IndexArgs& args)
      : a(args), p(*args.p), a_dct(p.algos & 1), a_fdct(p.algos & 2), a_orb(p.algos & 4), a_color(p.algos & 8),
        feats(a_fdct || a_orb), rs(p.resize_longest_side), cap(p.kp_cap) {
    span1 = (size_t)(a.h - 1) * a.row_stride + (size_t)a.w * a.channels;
    // chunks of up to 8 GB of input (16384 images): the colour leg runs one lane per image, so its rate grows with the
    // chunk (0.43 s for anything up to 4096 images, 0.48 s for 16384)
    per_chunk = std::max<size_t>(1, ((size_t)8192 << 20) / std::max(a.img_stride, span1));
    // A reflection search (mirror_mask != 0) runs every stage on the V views of each uploaded image: result i*V + v.  The
    // chunk shrinks by V so that the per-result buffers stay the size they have without views.
    // The views that swap width and height (bits 8..64) are a second geometry: their planes and colour images follow
    // the others' in the same buffers.
    Va = 1 + (size_t)__builtin_popcount((unsigned)a.view_mask & 7u);
    T = (size_t)__builtin_popcount((unsigned)a.view_mask >> 3);
    V = Va + T;
    views = V > 1, color_views = views && a_color && a.channels != 1;
    per_chunk = std::min<size_t>(std::min(std::max<size_t>(1, per_chunk / V), a.n), 16384 / V);
    per_out = per_chunk * V;  // results per chunk
    const size_t src_bytes = (per_chunk - 1) * a.img_stride + span1;
    // the reflected colour images follow the upload in the same buffer: the colour leg takes one base and per-image offsets
    cview_off = color_views ? (src_bytes + 255) & ~(size_t)255 : src_bytes;
    cview_bytes = (size_t)a.w * a.h * a.channels;
    tview_off = (cview_off + (color_views ? per_chunk * (Va - 1) * cview_bytes : 0) + 255) & ~(size_t)255;
    tgray_off = (per_chunk * Va * (size_t)a.w * a.h + 255) & ~(size_t)255;
    slot = feats ? (size_t)rs * rs + 16 : 0;  // room per image in the packed resize buffer
  }

  void lap(const char* what) {
    if (!trace) return;
    (void)hipStreamSynchronize(s.s);
    const auto t = std::chrono::steady_clock::now();
    fprintf(stderr, "[cbh_index_images] %-18s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(t - t_last).count());
    t_last = t;
  }

  int allocate() {
    for (hipError_t e : {s.err, s2.err, ev_up.err})
      if (e != hipSuccess) return cbh::fail("index_images streams", e);
    const size_t w = (size_t)a.w, h = (size_t)a.h;
    if (color_views && T)
      CBH_HIP(blocks.get(&d_src, tview_off + per_chunk * T * cview_bytes));
    else
      CBH_HIP(blocks.get(&d_src, cview_off + (color_views ? per_chunk * (V - 1) * cview_bytes : 0)));
    if (a.channels != 1 || views) CBH_HIP(blocks.get(&d_gray, T ? tgray_off + per_chunk * T * w * h : per_out * w * h));
    CBH_HIP(blocks.get(&d_out, per_out * sizeof(uint64_t)));
    CBH_HIP(blocks.get(&d_rects, per_out * 4 * sizeof(int)));
    if (feats) {
      CBH_HIP(blocks.get(&d_res, 2 * per_out * slot));  // the chunk-wide pass + the odd images redone
      CBH_HIP(blocks.get(&d_kp, per_out * (size_t)cap * sizeof(cbh_keypoint)));
      CBH_HIP(blocks.get(&d_cnt, per_out * sizeof(uint32_t)));
      if (a_orb) {
        CBH_HIP(blocks.get(&d_after, per_out * (size_t)cap * 2 * sizeof(float)));
        CBH_HIP(blocks.get(&d_desc, per_out * (size_t)cap * 32));
      }
      if (a_fdct) CBH_HIP(blocks.get(&d_kph, per_out * (size_t)cap * sizeof(uint64_t)));
    }
    if (a_color && a.channels != 1) {
      CBH_HIP(blocks.get(&d_cdesc, per_out * 258));
      CBH_HIP(blocks.get(&d_cok, per_out));
    }
    hr.resize(per_out * 4);
    off.resize(per_out), coff.resize(per_out);
    ws.resize(per_out), hs.resize(per_out), cnt.resize(per_out), kp_first.resize(per_out + 1), out_first.resize(per_out + 1);
    cw.assign(per_out, (uint32_t)a.w), chh.assign(per_out, (uint32_t)a.h), cst.assign(per_out, (uint32_t)a.row_stride);
    return CBH_OK;
  }

  // upload images i0 .. i0 + mu and make their grey planes (the views' planes)
  int upload_gray(size_t i0) {
    mu = std::min(per_chunk, a.n - i0);
    mt = mu * V, o0 = i0 * V;
    lap("(setup)");
    CBH_HIP(hipMemcpyAsync(d_src, a.imgs + i0 * a.img_stride, (mu - 1) * a.img_stride + span1, hipMemcpyHostToDevice, s.s));
    lap("upload");
    gray0 = d_src, gs0 = a.row_stride, gi0 = a.img_stride;
    int rc = CBH_OK;
    if (views)
      rc = cbh_gray_views_dev(d_src, mu, a.w, a.h, a.row_stride, a.img_stride, a.channels, a.view_mask & 7, d_gray,
                              color_views ? d_src + cview_off : nullptr, a.device, s.s);
    else if (a.channels != 1)
      rc = cbh_bgr2gray_dev(d_src, mt, a.w, a.h, a.row_stride, a.img_stride, a.channels, d_gray, a.device, s.s);
    if (rc == CBH_OK && T)
      rc = cbh_turn_views_dev(d_src, mu, a.w, a.h, a.row_stride, a.img_stride, a.channels, a.view_mask & 120,
                              d_gray + tgray_off, color_views ? d_src + tview_off : nullptr, a.device, s.s);
    if (views || a.channels != 1) gray0 = d_gray, gs0 = (size_t)a.w, gi0 = (size_t)a.w * a.h;
    return rc;
  }

  // The stages after the grey step take planes of one geometry: pass 0 the w x h views, pass 1 the h x w ones (false: the
  // call has none).  Plane j of a pass is view vfirst + j % vg of image j / vg.
  bool select(int pass) {
    if (pass == 0)
      vfirst = 0, vg = Va, gw = a.w, gh = a.h, gray = gray0, gs = gs0, gi = gi0;
    else
      vfirst = Va, vg = T, gw = a.h, gh = a.w, gray = d_gray + tgray_off, gs = (size_t)a.h, gi = (size_t)a.w * a.h;
    m = mu * vg;
    return m != 0;
  }
  bool contiguous() const { return vg == V; }  // the pass's results are rows o0 .. o0 + m
  size_t row(size_t j) const { return o0 + (j / vg) * V + vfirst + j % vg; }

  // The colour descriptor is made from the ORIGINAL colour image (scanner.cpp:868-872); grey input: "passed a grayscale
  // image", the descriptor stays empty.
  // It runs on its own stream from a helper thread: the clustering kernel is one lane per image (a few dozen waves with
  // long sequential chains), so it occupies a sliver of the chip for a long time -- the other stages, with their host
  // synchronisations, run beside it.
  int start_color() {
    color_rc = CBH_OK;
    if (!a_color) return CBH_OK;
    if (a.channels == 1) {
      memset(a.color_descs + o0 * 258, 0, mt * 258);
      memset(a.color_ok + o0, 0, mt);
      return CBH_OK;
    }
    CBH_HIP(hipEventRecord(ev_up.ev, s.s));
    for (size_t i = 0; i < mu; ++i)
      for (size_t v = 0; v < V; ++v) {  // view 0 is the upload itself; the reflections were written behind it, then the turns
        const bool turned = v >= Va;
        coff[i * V + v] = v == 0   ? i * a.img_stride
                          : turned ? tview_off + (i * T + v - Va) * cview_bytes
                                   : cview_off + (i * (Va - 1) + v - 1) * cview_bytes;
        cw[i * V + v] = (uint32_t)(turned ? a.h : a.w), chh[i * V + v] = (uint32_t)(turned ? a.w : a.h);
        cst[i * V + v] = (uint32_t)(v == 0 ? a.row_stride : (size_t)cw[i * V + v] * a.channels);
      }
    color_thread.t = std::thread([this] {
      cbh::DeviceGuard tg(a.device);
      hipError_t e = hipStreamWaitEvent(s2.s, ev_up.ev, 0);
      if (e == hipSuccess)
        color_rc = cbh_color_descriptors_dev(d_src, mt, coff.data(), cw.data(), chh.data(), cst.data(), a.channels, d_cdesc,
                                             d_cok, a.device, s2.s);
      if (e == hipSuccess && color_rc == CBH_OK &&
          ((e = hipMemcpyAsync(a.color_descs + o0 * 258, d_cdesc, mt * 258, hipMemcpyDeviceToHost, s2.s)) != hipSuccess ||
           (e = hipMemcpyAsync(a.color_ok + o0, d_cok, mt, hipMemcpyDeviceToHost, s2.s)) != hipSuccess ||
           (e = hipStreamSynchronize(s2.s)) != hipSuccess))
        ;
      if (e != hipSuccess) {
        cbh::set_last_error("index_images colour leg", e);
        color_rc = CBH_E_HIP;
      }
    });
    return CBH_OK;
  }
  int finish_color() {
    color_thread.join();
    return color_rc;
  }

  // `if (_params.algos && _params.autocrop) autocrop(cvGray, 20)`, and the launch plan of the per-geometry stages
  // (hash, resize): mode first (cbh_regions.h)
  int kept_regions() {
    const int rc = cbh::fetch_kept_regions(gray, m, gw, gh, gs, gi, p.autocrop_range, d_rects, hr.data(), a.device, s.s);
    if (rc) return rc;
    if (a.rects && contiguous()) memcpy(a.rects + o0 * 4, hr.data(), m * 4 * sizeof(int));
    else if (a.rects)
      for (size_t i = 0; i < m; ++i) memcpy(a.rects + row(i) * 4, hr.data() + i * 4, 4 * sizeof(int));
    lap("gray + autocrop");
    cbh::plan_regions(hr.data(), m, true, &plan);
    return CBH_OK;
  }

  int hash() {
    if (a_dct) {
      for (const cbh::RegionRun& r : plan) {
        const int rc = cbh::launch_dcthash_kept(gray + r.first * gi, r.count, gw, gh, gs, gi, r.rect, d_out + r.first, s.s);
        if (rc) return rc;
      }
      if (contiguous()) {
        CBH_HIP(hipMemcpyAsync(a.dct_hashes + o0, d_out, m * sizeof(uint64_t), hipMemcpyDeviceToHost, s.s));
      } else {
        hd.resize(m);
        CBH_HIP(hipMemcpyAsync(hd.data(), d_out, m * sizeof(uint64_t), hipMemcpyDeviceToHost, s.s));
        CBH_HIP(hipStreamSynchronize(s.s));
        for (size_t i = 0; i < m; ++i) a.dct_hashes[row(i)] = hd[i];
      }
    }
    lap("dct hash");
    return CBH_OK;
  }

  // sizeLongestSide(cvGray, 400) of each kept region with the same launch plan; the resized images are packed back to
  // back (ORB and the keypoint hashes take per-image offsets), an odd image in its own slot behind the chunk-wide pass
  int resize() {
    cbh::pack_resized(plan, rs, ws.data(), hs.data(), off.data(), &base);
    for (size_t k = 0; k < plan.size(); ++k) {
      const cbh::RegionRun& r = plan[k];
      int dw, dh;
      const int rc = cbh::resize_kept(gray + r.first * gi, r.count, gs, gi, r.rect, rs, d_res + base[k], a.device, s.s, &dw, &dh);
      if (rc) return rc;
    }
    lap("resize");
    if (a.resized_dims)
      for (size_t i = 0; i < m; ++i) a.resized_dims[2 * row(i)] = (int)ws[i], a.resized_dims[2 * row(i) + 1] = (int)hs[i];
    return CBH_OK;
  }

  int orb() {
    // images the resize rejected get a 1x1 stand-in geometry: no pyramid level, no keypoints
    ow.assign(ws.begin(), ws.begin() + m), oh.assign(hs.begin(), hs.begin() + m);
    for (size_t i = 0; i < m; ++i)
      if (ow[i] == 0) ow[i] = oh[i] = 1, off[i] = 0;
    const int rc = cbh_orb_dev(d_res, m, off.data(), ow.data(), oh.data(), ow.data(), p.num_features, cap, d_kp,
                               a_orb ? d_after : nullptr, a_orb ? d_desc : nullptr, d_cnt, a.device, s.s);
    if (rc) return rc;
    lap("orb");
    const size_t per = m * (size_t)cap;
    hkp.resize(per);
    CBH_HIP(hipMemcpyAsync(cnt.data(), d_cnt, m * sizeof(uint32_t), hipMemcpyDeviceToHost, s.s));
    CBH_HIP(hipMemcpyAsync(hkp.data(), d_kp, per * sizeof(cbh_keypoint), hipMemcpyDeviceToHost, s.s));
    if (a_orb) {
      hafter.resize(per * 2);
      CBH_HIP(hipMemcpyAsync(hafter.data(), d_after, per * 2 * sizeof(float), hipMemcpyDeviceToHost, s.s));
      if (!contiguous()) hdesc.resize(per * 32);
      CBH_HIP(hipMemcpyAsync(contiguous() ? a.desc + o0 * (size_t)cap * 32 : hdesc.data(), d_desc, per * 32,
                             hipMemcpyDeviceToHost, s.s));
    }
    CBH_HIP(hipStreamSynchronize(s.s));
    if (a_orb && !contiguous())
      for (size_t i = 0; i < m; ++i) memcpy(a.desc + row(i) * cap * 32, hdesc.data() + i * cap * 32, (size_t)cap * 32);
    lap("orb download");
    // the keypoint list as processImage holds it after makeKeyPointDescriptors (which rewrites pt) -- or as detected
    for (size_t i = 0; i < m; ++i) {
      a.kp_counts[row(i)] = cnt[i];
      const size_t c = std::min<size_t>(cnt[i], (size_t)cap);
      for (size_t j = 0; j < c; ++j) {
        cbh_keypoint k = hkp[i * cap + j];
        if (a_orb) k.x = hafter[2 * (i * cap + j)], k.y = hafter[2 * (i * cap + j) + 1];
        a.kp[row(i) * cap + j] = k;
      }
    }
    lap("keypoint lists");
    return CBH_OK;
  }

  int keypoint_hashes() {
    tri.clear();
    kp_first[0] = 0;
    for (size_t i = 0; i < m; ++i) {
      const size_t c = std::min<size_t>(cnt[i], (size_t)cap);
      for (size_t j = 0; j < c; ++j) {
        const cbh_keypoint& k = a.kp[row(i) * cap + j];
        tri.push_back(k.x), tri.push_back(k.y), tri.push_back(k.size);
      }
      kp_first[i + 1] = (uint32_t)(tri.size() / 3);
    }
    lap("kp triples");
    const int rc = cbh_keypoint_hashes_dev(d_res, m, off.data(), ow.data(), oh.data(), ow.data(), tri.data(), kp_first.data(),
                                           d_kph, out_first.data(), a.device, s.s);
    if (rc) return rc;
    lap("kp hashes");
    const size_t total = out_first[m];
    hh.resize(std::max<size_t>(total, 1));
    if (total) CBH_HIP(hipMemcpyAsync(hh.data(), d_kph, total * sizeof(uint64_t), hipMemcpyDeviceToHost, s.s));
    CBH_HIP(hipStreamSynchronize(s.s));
    for (size_t i = 0; i < m; ++i) {
      const uint32_t c = out_first[i + 1] - out_first[i];
      a.kph_counts[row(i)] = c;
      memcpy(a.kp_hashes + row(i) * cap, hh.data() + out_first[i], (size_t)c * sizeof(uint64_t));
    }
    return CBH_OK;
  }
};

// the stages after the grey step and the colour leg's start, on the planes select() chose
int run_pass(IndexCall& c, bool feats, bool a_fdct) {
  int rc;
  if ((rc = c.kept_regions()) || (rc = c.hash())) return rc;
  if (!feats) {
    CBH_HIP(hipStreamSynchronize(c.s.s));
    return CBH_OK;
  }
  if ((rc = c.resize()) || (rc = c.orb()) || (a_fdct && (rc = c.keypoint_hashes()))) return rc;
  return CBH_OK;
}

int index_images_one(const IndexArgs& a, int max_mask) {
  if (!cbh::device_usable(a.device)) return CBH_E_NODEVICE;
  const cbh_index_params* p = a.p;
  if (!p || a.view_mask < 0 || a.view_mask > max_mask) return CBH_E_INVAL;
  const bool a_dct = p->algos & 1, a_fdct = p->algos & 2, a_orb = p->algos & 4, a_color = p->algos & 8;
  const bool feats = a_fdct || a_orb;
  const int rs = p->resize_longest_side, cap = p->kp_cap;
  if (a.n == 0) return CBH_OK;
  if (!a.imgs || a.w <= 0 || a.h <= 0 || (a.channels != 1 && a.channels != 3 && a.channels != 4) ||
      a.row_stride < (size_t)a.w * a.channels || (a_dct && !a.dct_hashes) ||
      (feats && (rs < 1 || rs > 8192 || cap < 1 || p->num_features < 0 || !a.kp_counts || !a.kp)) || (a_orb && !a.desc) ||
      (a_fdct && (!a.kph_counts || !a.kp_hashes)) || (a_color && (!a.color_descs || !a.color_ok)))
    return CBH_E_INVAL;
  cbh::DeviceGuard g(a.device);
  if (!g.ok) return CBH_E_NODEVICE;
  IndexCall c(a);
  int rc = c.allocate();
  for (size_t i0 = 0; rc == CBH_OK && i0 < a.n; i0 += c.per_chunk) {
    if ((rc = c.upload_gray(i0)) || (rc = c.start_color())) break;
    for (int pass = 0; pass < 2 && rc == CBH_OK; ++pass)
      if (c.select(pass)) rc = run_pass(c, feats, a_fdct);
    if (rc) break;
    rc = c.finish_color();
  }
  return rc;
}

}  // namespace

// A large batch without the colour leg is cut into a few sub-batches that run on their own host threads and streams: one
// uploads while another computes (host in / host out, 4096 BGR images 640x480, hash + ORB + keypoint hashes: 156 -> 122
// ms).  The colour leg wants ONE big batch (a lane per image), so calls that include it stay whole.
extern "C" int cbh_index_images(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                                int channels, const cbh_index_params* p, uint64_t* dct_hashes, int32_t* rects,
                                int32_t* resized_dims, uint32_t* kp_counts, cbh_keypoint* kp, uint8_t* desc,
                                uint32_t* kph_counts, uint64_t* kp_hashes, uint8_t* color_descs, uint8_t* color_ok,
                                int device) {
  static const int max_threads = [] {
    const char* e = getenv("CBH_PIPELINE_THREADS");
    const int v = e ? atoi(e) : 4;
    return v < 1 ? 1 : (v > 16 ? 16 : v);
  }();
  const IndexArgs whole{imgs, n, w, h, row_stride, img_stride, channels, 0, p, dct_hashes, rects, resized_dims, kp_counts,
                        kp, desc, kph_counts, kp_hashes, color_descs, color_ok, device};
  const bool split_ok = p && n >= 1024 && !(p->algos & 8) && (p->algos & 6) && imgs && img_stride > 0;
  const size_t T = split_ok ? std::min<size_t>((size_t)max_threads, n / 512) : 1;
  if (T <= 1) return index_images_one(whole, 0);
  std::vector<int> rc(T, CBH_OK);
  std::vector<std::thread> th;
  const size_t cap = p->kp_cap > 0 ? (size_t)p->kp_cap : 0;
  for (size_t t = 0; t < T; ++t) {
    const size_t a = t * n / T, b = (t + 1) * n / T;
    th.emplace_back([&, t, a, b]() {
      IndexArgs part = whole;
      part.imgs = imgs + a * img_stride, part.n = b - a;
      part.dct_hashes = dct_hashes ? dct_hashes + a : nullptr, part.rects = rects ? rects + 4 * a : nullptr;
      part.resized_dims = resized_dims ? resized_dims + 2 * a : nullptr, part.kp_counts = kp_counts ? kp_counts + a : nullptr;
      part.kp = kp ? kp + a * cap : nullptr, part.desc = desc ? desc + a * cap * 32 : nullptr;
      part.kph_counts = kph_counts ? kph_counts + a : nullptr, part.kp_hashes = kp_hashes ? kp_hashes + a * cap : nullptr;
      rc[t] = index_images_one(part, 0);
    });
  }
  for (auto& x : th) x.join();
  for (int r : rc)
    if (r != CBH_OK) return r;
  return CBH_OK;
}

// Engine::query's reflection search (src/engine.cpp:423-436): processImage of the needle and of Engine::mirrored(needle,
// h, v) (:357-365) for the bits of mirrorMask, from one upload per chunk.  Runs whole (no threaded split): its results
// are the same either way, and the colour leg would keep it whole anyway.
extern "C" int cbh_index_images_views(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                                      int channels, int mirror_mask, const cbh_index_params* p, uint64_t* dct_hashes,
                                      int32_t* rects, int32_t* resized_dims, uint32_t* kp_counts, cbh_keypoint* kp,
                                      uint8_t* desc, uint32_t* kph_counts, uint64_t* kp_hashes, uint8_t* color_descs,
                                      uint8_t* color_ok, int device) {
  return index_images_one(IndexArgs{imgs, n, w, h, row_stride, img_stride, channels, mirror_mask, p, dct_hashes, rects,
                                    resized_dims, kp_counts, kp, desc, kph_counts, kp_hashes, color_descs, color_ok, device},
                          7);
}

// The same for all eight views: the quarter turns and transposes of the needle (bits 8..64, turns.hip) beside the
// reflections, still from one upload per chunk.
extern "C" int cbh_index_images_views_ex(const uint8_t* imgs, size_t n, int w, int h, size_t row_stride, size_t img_stride,
                                         int channels, int view_mask, const cbh_index_params* p, uint64_t* dct_hashes,
                                         int32_t* rects, int32_t* resized_dims, uint32_t* kp_counts, cbh_keypoint* kp,
                                         uint8_t* desc, uint32_t* kph_counts, uint64_t* kp_hashes, uint8_t* color_descs,
                                         uint8_t* color_ok, int device) {
  return index_images_one(IndexArgs{imgs, n, w, h, row_stride, img_stride, channels, view_mask, p, dct_hashes, rects,
                                    resized_dims, kp_counts, kp, desc, kph_counts, kp_hashes, color_descs, color_ok, device},
                          127);
}
