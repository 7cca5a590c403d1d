// Host-only: the error plumbing of the C ABI and the owners of device and pinned host memory.  Needs the HIP runtime API and nothing from the
// kernel headers, so a plain host compiler can build it against a stand-in runtime (tests/cpp/fake/test_devbuf.cpp).
#pragma once
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/apdgicp_hip.h"

namespace apd {

inline thread_local std::string g_last_error;
inline int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}

#define APD_HIP(expr)                                                                                         \
  do {                                                                                                        \
    hipError_t e_ = (expr);                                                                                   \
    if (e_ != hipSuccess)                                                                                     \
      return fail(APDGICP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" __FILE__ ":" + std::to_string(__LINE__) + ")"); \
  } while (0)
#define APD_TRY(expr)          \
  do {                         \
    int rc_ = (expr);          \
    if (rc_ < 0) return rc_;   \
  } while (0)

// One allocation of device memory (hipMalloc) or of pinned host memory (hipHostMalloc), owned: the destructor frees it, a move leaves the
// source empty, there is no copy.  An owner therefore lists none of its buffers in its destructor; what it has to do there is wait for the
// streams that may still use them, before its members go.  `live` counts the allocations of the kind that exist in the process
// (apdgicp_debug_live_buffers): up where an allocation succeeds, down where a pointer is freed.  Pinned memory that is still a raw pointer
// (the engine's poll records, which two slots hand to each other) is not counted.
template <bool Pinned>
struct OwnedBuf {
  void* p = nullptr;
  size_t cap = 0;
  inline static std::atomic<long long> live{0};
  OwnedBuf() = default;
  OwnedBuf(const OwnedBuf&) = delete;
  OwnedBuf& operator=(const OwnedBuf&) = delete;
  OwnedBuf(OwnedBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p, cap = o.cap;
      o.p = nullptr, o.cap = 0;
    }
    return *this;
  }
  ~OwnedBuf() { release(); }
  // at least `bytes`: keeps what it has when that is enough, else frees it and allocates anew (the contents are lost).  Device sizes are
  // rounded up to 256 bytes, pinned ones are taken as they come (the callers bring their own head room).
  int ensure(size_t bytes) {
    if (bytes <= cap) return 0;
    release();
    const size_t want = Pinned ? bytes : (bytes + 255) & ~size_t(255);
    if constexpr (Pinned) APD_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    else APD_HIP(hipMalloc(&p, want));
    live++;
    cap = want;
    return 0;
  }
  void release() {
    if (p) {
      hipError_t e = Pinned ? hipHostFree(p) : hipFree(p);
      (void)e;
      live--;
    }
    p = nullptr;
    cap = 0;
  }
  template <typename T>
  T* as() const { return (T*)p; }
};
using DevBuf = OwnedBuf<false>;
using PinnedBuf = OwnedBuf<true>;

// A small host->device table that is re-uploaded only when its contents change.  A changed table goes through one of two
// pinned staging buffers and an asynchronous copy on the caller's stream -- stream order already keeps it behind the
// kernels that still read the old contents -- and the host never waits for the GPU: a staging buffer is only rewritten
// after the event recorded behind ITS last copy has fired (normally long ago).
struct CachedTable {
  DevBuf dev;
  std::vector<char> host;  // last uploaded contents (for the comparison)
  PinnedBuf pin[2];
  hipEvent_t ev[2] = {nullptr, nullptr};
  int cur = 0;
  ~CachedTable() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int upload(const void* data, size_t bytes, hipStream_t stream) {
    if (dev.p && host.size() == bytes && (bytes == 0 || memcmp(host.data(), data, bytes) == 0)) return 0;
    host.assign((const char*)data, (const char*)data + bytes);
    if (std::max<size_t>(bytes, 16) > dev.cap) APD_HIP(hipStreamSynchronize(stream));  // the old device buffer is about to be freed
    APD_TRY(dev.ensure(std::max<size_t>(bytes, 16)));
    if (!bytes) return 0;
    cur ^= 1;
    if (!ev[cur]) APD_HIP(hipEventCreateWithFlags(&ev[cur], hipEventDisableTiming));
    else APD_HIP(hipEventSynchronize(ev[cur]));
    if (bytes > pin[cur].cap) APD_TRY(pin[cur].ensure(std::max<size_t>(bytes * 2, 256)));
    memcpy(pin[cur].p, data, bytes);
    APD_HIP(hipMemcpyAsync(dev.p, pin[cur].p, bytes, hipMemcpyHostToDevice, stream));
    APD_HIP(hipEventRecord(ev[cur], stream));
    return 0;
  }
  template <typename T>
  T* as() const { return (T*)dev.p; }
  CachedTable() = default;
  CachedTable(const CachedTable&) = delete;
  CachedTable& operator=(const CachedTable&) = delete;
};

}  // namespace apd
