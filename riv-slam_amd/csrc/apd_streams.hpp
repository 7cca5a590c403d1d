// Where the registration engine's HIP streams come from: one registry per process, counted per device.
//
// The HIP runtime multiplexes the streams of a process onto GPU_MAX_HW_QUEUES hardware queues (4 by default) PER STREAM PRIORITY,
// and two streams that share a queue run their launches one behind the other.  The null stream, torch's streams and RCCL's live in
// the pool of the normal priority, so an engine stream created there lands wherever creation order leaves it -- with four handles
// (or one pooled Levenberg-Marquardt handle, four streams) in flight that costs a quarter of the throughput (docs/experiments.md).
// The registry therefore creates the engine's streams in ONE other class while fewer than Q of them live on the device, and as
// plain normal-priority streams beyond that or where the device has a single priority level.  Q is read from GPU_MAX_HW_QUEUES and
// never set here; destroying a stream frees its slot.
//
// This header is the policy only and has no HIP in it: creation and destruction are injected (Engine binds them to hipStreamCreate*
// in apd_engine.hpp, tests/cpp/test_stream_slots.cpp to counters), a stream is a void*.
#pragma once
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <unordered_map>
#include <utility>

namespace apd {

enum class StreamClass { Normal = 0, Low, High };

// APDGICP_STREAM_CLASS=normal|low|high (A/B runs; `normal` is creation in the caller's own class, as before the registry).
// Unset or empty: `dflt`.  Anything else is refused.
inline bool parse_stream_class(const char* v, StreamClass dflt, StreamClass* out) {
  if (!v || !*v) return *out = dflt, true;
  if (!strcmp(v, "normal")) return *out = StreamClass::Normal, true;
  if (!strcmp(v, "low")) return *out = StreamClass::Low, true;
  if (!strcmp(v, "high")) return *out = StreamClass::High, true;
  return false;
}

// Q: the value of GPU_MAX_HW_QUEUES as the runtime will read it; the runtime's default of 4 when unset, not a number or not positive.
inline int hw_queue_limit(const char* v) {
  constexpr int kRuntimeDefault = 4;
  if (!v || !*v) return kRuntimeDefault;
  char* end = nullptr;
  const long q = strtol(v, &end, 10);
  if (end == v || *end != '\0' || q <= 0 || q > 1 << 20) return kRuntimeDefault;
  return (int)q;
}

class StreamSlots {
 public:
  struct Backend {
    // a stream of class `cls` on `device` into *out; 0 or an error code that acquire() hands back
    std::function<int(int device, StreamClass cls, void** out)> create;
    std::function<void(int device, void* stream)> destroy;
    // whether `device` has more than one stream priority level (Low / High mean nothing otherwise)
    std::function<bool(int device)> has_priorities;
  };
  StreamSlots(Backend be, StreamClass cls, int q) : be_(std::move(be)), cls_(cls), limit_(q) {}

  StreamClass stream_class() const { return cls_; }
  int limit() const { return limit_; }

  int acquire(int device, void** out) {
    std::lock_guard<std::mutex> lk(mu_);
    int& live = placed_[device];
    const bool place = cls_ != StreamClass::Normal && live < limit_ && be_.has_priorities(device);
    void* s = nullptr;
    const int rc = be_.create(device, place ? cls_ : StreamClass::Normal, &s);
    if (rc != 0) return rc;
    if (place) live++;
    owned_[s] = {device, place};
    *out = s;
    return 0;
  }

  // a stream acquire() did not hand out is left alone (false)
  bool release(void* s) {
    std::lock_guard<std::mutex> lk(mu_);
    auto it = owned_.find(s);
    if (it == owned_.end()) return false;
    const Owned o = it->second;
    owned_.erase(it);
    if (o.placed) placed_[o.device]--;
    be_.destroy(o.device, s);
    return true;
  }

  int placed(int device) {
    std::lock_guard<std::mutex> lk(mu_);
    return placed_[device];
  }
  int live() {
    std::lock_guard<std::mutex> lk(mu_);
    return (int)owned_.size();
  }

 private:
  struct Owned {
    int device;
    bool placed;
  };
  Backend be_;
  const StreamClass cls_;
  const int limit_;
  std::mutex mu_;
  std::map<int, int> placed_;  // device -> live streams outside the normal class
  std::unordered_map<void*, Owned> owned_;
};

}  // namespace apd
