// cbh_staging.h -- internal: what the entry points that take HOST memory share.  Each of them uploads its inputs, calls
// its _dev twin (or a launcher) on a stream of the library's own, fetches the results and leaves nothing behind.
// Include after cbh_internal.h: the allocations below go through its hipMalloc gate (fault injection).
#pragma once
#include <string>
#include <vector>

#include "cbh_internal.h"

namespace cbh {

// The life of one host-memory call: a non-blocking stream `s`, the device buffers taken with alloc(), and the first HIP
// error.  After an error alloc / up / down / sync do nothing, so a body reads straight down and asks status() where it
// has to decide.  Whichever way the call returns, the destructor waits for the stream, frees the buffers and destroys
// the stream, in that order: nothing that was queued can still touch a buffer, and the caller finds the stream drained.
// Declare it after the DeviceGuard (it must leave first) and before anything that gives scratch back to `s`.
struct Staging {
  hipStream_t s = nullptr;
  explicit Staging(const char* entry) : entry_(entry) { err_ = hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
  Staging(const Staging&) = delete;
  Staging& operator=(const Staging&) = delete;
  ~Staging() {
    if (s) (void)hipStreamSynchronize(s);
    while (n_ > 0) (void)hipFree(bufs_[--n_]);
    if (s) stream_destroy(s);
  }
  template <class T>
  void alloc(T** p, size_t bytes) {
    *p = nullptr;
    if (err_ != hipSuccess) return;
    if (n_ == kMost) {
      err_ = hipErrorInvalidValue;
    } else if ((err_ = hipMalloc(p, bytes)) == hipSuccess) {
      bufs_[n_++] = *p;
    }
  }
  void up(void* d, const void* h, size_t bytes) {
    if (err_ == hipSuccess) note("upload", hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, s));
  }
  void down(void* h, const void* d, size_t bytes) {
    if (err_ == hipSuccess) note("fetch", hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, s));
  }
  void sync() {
    if (err_ == hipSuccess) note("fetch", hipStreamSynchronize(s));
  }
  // CBH_OK, or the code of the first error with "<entry point> <stage>" as the error text
  int status() const { return err_ == hipSuccess ? CBH_OK : fail((std::string(entry_) + ' ' + stage_).c_str(), err_); }

 private:
  static constexpr int kMost = 8;
  void note(const char* stage, hipError_t e) {
    if ((err_ = e) != hipSuccess) stage_ = stage;
  }
  const char* entry_;
  const char* stage_ = "setup";
  hipError_t err_;
  void* bufs_[kMost];
  int n_ = 0;
};

}  // namespace cbh
