// Stand-alone test of the stream registry's POLICY (riv-slam_amd/csrc/apd_streams.hpp) with counters in place of HIP: fill to Q, overflow to
// the normal class, release and reuse, Q from the environment's value, a device with one priority level, and eight threads
// acquiring and releasing at once.  Built with -fsanitize=thread and -fsanitize=address,undefined by tests/test_stream_slots.py; prints "ok 1".
#include <atomic>
#include <cstdio>
#include <thread>
#include <vector>

#include "apd_streams.hpp"

using apd::StreamClass;
using apd::StreamSlots;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

namespace {

// what the fake runtime has live, by the class it was asked for; a "stream" is a heap int holding that class (a leak or a double
// destroy is an AddressSanitizer report)
struct Fake {
  std::atomic<int> live[3] = {{0}, {0}, {0}};
  std::atomic<int> peak_placed{0};
  std::atomic<int> fail_next{0};
  bool priorities = true;

  StreamSlots::Backend backend() {
    StreamSlots::Backend be;
    be.create = [this](int, StreamClass c, void** out) -> int {
      if (fail_next.exchange(0)) return -7;
      *out = new int((int)c);
      const int n = ++live[(int)c];
      if (c != StreamClass::Normal) {
        int p = peak_placed.load();
        while (n > p && !peak_placed.compare_exchange_weak(p, n)) {
        }
      }
      return 0;
    };
    be.destroy = [this](int, void* s) {
      int* p = (int*)s;
      --live[*p];
      delete p;
    };
    be.has_priorities = [this](int) { return priorities; };
    return be;
  }
  int total() const { return live[0] + live[1] + live[2]; }
};

StreamClass class_of(void* s) { return (StreamClass) * (int*)s; }

int test_environment_values() {
  CHECK(apd::hw_queue_limit(nullptr) == 4);
  CHECK(apd::hw_queue_limit("") == 4);
  CHECK(apd::hw_queue_limit("8") == 8);
  CHECK(apd::hw_queue_limit("32") == 32);
  CHECK(apd::hw_queue_limit("1") == 1);
  CHECK(apd::hw_queue_limit("0") == 4);
  CHECK(apd::hw_queue_limit("-3") == 4);
  CHECK(apd::hw_queue_limit("eight") == 4);
  CHECK(apd::hw_queue_limit("8x") == 4);
  CHECK(apd::hw_queue_limit("99999999999999999999") == 4);
  StreamClass c = StreamClass::Normal;
  CHECK(apd::parse_stream_class(nullptr, StreamClass::Low, &c) && c == StreamClass::Low);
  CHECK(apd::parse_stream_class("", StreamClass::High, &c) && c == StreamClass::High);
  CHECK(apd::parse_stream_class("normal", StreamClass::Low, &c) && c == StreamClass::Normal);
  CHECK(apd::parse_stream_class("low", StreamClass::Normal, &c) && c == StreamClass::Low);
  CHECK(apd::parse_stream_class("high", StreamClass::Low, &c) && c == StreamClass::High);
  CHECK(!apd::parse_stream_class("mask", StreamClass::Low, &c));
  CHECK(!apd::parse_stream_class("Low", StreamClass::Low, &c));
  CHECK(!apd::parse_stream_class("lowest", StreamClass::Low, &c));
  return 0;
}

int test_fill_overflow_reuse() {
  Fake f;
  StreamSlots reg(f.backend(), StreamClass::Low, 4);
  std::vector<void*> s(7, nullptr);
  for (int i = 0; i < 7; i++) {
    CHECK(reg.acquire(0, &s[i]) == 0 && s[i]);
    CHECK(class_of(s[i]) == (i < 4 ? StreamClass::Low : StreamClass::Normal));  // fill to Q, then the normal class
  }
  CHECK(reg.placed(0) == 4 && reg.live() == 7 && f.live[(int)StreamClass::Low] == 4 && f.live[(int)StreamClass::Normal] == 3);
  // another device counts for itself
  void* d1 = nullptr;
  CHECK(reg.acquire(1, &d1) == 0 && class_of(d1) == StreamClass::Low && reg.placed(1) == 1 && reg.placed(0) == 4);
  // releasing a normal-class stream frees no slot, releasing a placed one frees exactly one
  CHECK(reg.release(s[5]));
  void* t = nullptr;
  CHECK(reg.acquire(0, &t) == 0 && class_of(t) == StreamClass::Normal);
  CHECK(reg.release(t));
  CHECK(reg.release(s[1]) && reg.placed(0) == 3);
  CHECK(reg.acquire(0, &s[1]) == 0 && class_of(s[1]) == StreamClass::Low && reg.placed(0) == 4);
  CHECK(reg.acquire(0, &s[5]) == 0 && class_of(s[5]) == StreamClass::Normal);
  // a stream the registry did not hand out (the caller's own) is left alone, a second release too
  int callers = 0;
  CHECK(!reg.release(&callers));
  CHECK(reg.release(d1) && !reg.release(d1));
  // a failed creation takes no slot and hands the code back
  CHECK(reg.release(s[0]) && reg.placed(0) == 3);
  f.fail_next = 1;
  void* none = nullptr;
  CHECK(reg.acquire(0, &none) == -7 && none == nullptr && reg.placed(0) == 3);
  CHECK(reg.acquire(0, &s[0]) == 0 && class_of(s[0]) == StreamClass::Low);
  for (void* x : s) CHECK(reg.release(x));
  CHECK(reg.placed(0) == 0 && reg.live() == 0 && f.total() == 0 && f.peak_placed == 5);  // (four on device 0 and the one on device 1)
  return 0;
}

int test_classes() {
  {  // `normal`: nothing is placed, whatever Q
    Fake f;
    StreamSlots reg(f.backend(), StreamClass::Normal, 8);
    void* s[3];
    for (void*& x : s) CHECK(reg.acquire(0, &x) == 0 && class_of(x) == StreamClass::Normal);
    CHECK(reg.placed(0) == 0);
    for (void* x : s) CHECK(reg.release(x));
  }
  {  // a device with one priority level: today's streams
    Fake f;
    f.priorities = false;
    StreamSlots reg(f.backend(), StreamClass::High, 4);
    void* x = nullptr;
    CHECK(reg.acquire(0, &x) == 0 && class_of(x) == StreamClass::Normal && reg.placed(0) == 0);
    CHECK(reg.release(x));
  }
  {  // Q = 1
    Fake f;
    StreamSlots reg(f.backend(), StreamClass::Low, apd::hw_queue_limit("1"));
    void *a = nullptr, *b = nullptr;
    CHECK(reg.acquire(0, &a) == 0 && reg.acquire(0, &b) == 0 && class_of(a) == StreamClass::Low && class_of(b) == StreamClass::Normal);
    CHECK(reg.release(a) && reg.release(b));
  }
  return 0;
}

int test_threads() {
  Fake f;
  constexpr int Q = 4, kThreads = 8, kRounds = 400;
  StreamSlots reg(f.backend(), StreamClass::Low, Q);
  std::atomic<int> bad{0};
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; t++)
    th.emplace_back([&, t] {
      for (int r = 0; r < kRounds; r++) {
        void* s[3] = {nullptr, nullptr, nullptr};  // (a pooled handle takes several)
        const int n = 1 + (r + t) % 3;
        for (int i = 0; i < n; i++)
          if (reg.acquire(t % 2, &s[i]) != 0 || !s[i]) bad++;
        if (reg.placed(t % 2) > Q) bad++;
        for (int i = 0; i < n; i++)
          if (!reg.release(s[i])) bad++;
      }
    });
  for (auto& x : th) x.join();
  CHECK(bad == 0);
  CHECK(f.peak_placed <= 2 * Q);  // (two devices; per device the ceiling is checked in the loop)
  CHECK(reg.placed(0) == 0 && reg.placed(1) == 0 && reg.live() == 0 && f.total() == 0);
  // and the slots are all there again
  void* s[Q + 1];
  for (int i = 0; i <= Q; i++) CHECK(reg.acquire(0, &s[i]) == 0 && class_of(s[i]) == (i < Q ? StreamClass::Low : StreamClass::Normal));
  for (void* x : s) CHECK(reg.release(x));
  return 0;
}

}  // namespace

int main() {
  if (test_environment_values() || test_fill_overflow_reuse() || test_classes() || test_threads()) return 1;
  printf("ok 1\n");
  return 0;
}
