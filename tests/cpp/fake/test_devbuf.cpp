// TEST-ONLY: the owners of riv-slam_amd/csrc/apd_devbuf.hpp -- DevBuf, PinnedBuf, CachedTable::dev -- against the fake runtime of
// fake_backend.cpp, whose hipMalloc is malloc: under -fsanitize=address,undefined (tests/test_sanitizers.py) a double free or a use after free
// is a sanitizer report, and fake_live_allocations() counts what was never freed.  Prints "ok 1" and exits 0 only when nothing is left alive
// by the runtime's count and by the header's own two counters.
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "apd_devbuf.hpp"

extern "C" long fake_live_allocations();
extern "C" void fake_fail_allocations_after(long n);

using namespace apd;

static int g_bad = 0;
#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::printf("FAILED %s (%s:%d)\n", #cond, __FILE__, __LINE__);       \
      g_bad++;                                                             \
    }                                                                      \
  } while (0)

template <class Buf>
static void touch(Buf& b) {  // every byte the buffer says it has: an overrun or a freed block is a report
  if (b.p) std::memset(b.p, 0x5a, b.cap);
}

template <class Buf>
static void one_owner(bool rounds) {
  const long long live0 = Buf::live.load();
  {
    Buf a;
    CHECK(a.p == nullptr && a.cap == 0);
    CHECK(a.ensure(100) == 0 && a.p && a.cap == (rounds ? 256u : 100u));
    touch(a);
    CHECK(Buf::live.load() == live0 + 1);
    CHECK(a.ensure(1000) == 0 && a.cap == (rounds ? 1024u : 1000u));  // larger: the old block goes, one is alive
    touch(a);
    CHECK(Buf::live.load() == live0 + 1);
    void* before = a.p;
    CHECK(a.ensure(10) == 0 && a.p == before && a.cap >= 1000);  // smaller: nothing happens
    a.release();
    CHECK(a.p == nullptr && a.cap == 0 && Buf::live.load() == live0);
    a.release();  // (an empty one: nothing to free)
    CHECK(a.ensure(64) == 0 && a.p);
    touch(a);
    CHECK(a.template as<int>() == (int*)a.p);

    Buf b(std::move(a));  // move construction: the source is empty
    CHECK(a.p == nullptr && a.cap == 0 && b.p && b.cap >= 64);
    touch(b);
    Buf c;
    CHECK(c.ensure(300) == 0);
    void* bp = b.p;
    c = std::move(b);  // onto an owner: what it held is freed
    CHECK(c.p == bp && b.p == nullptr && b.cap == 0 && Buf::live.load() == live0 + 1);
    touch(c);
    Buf& self = c;
    c = std::move(self);  // onto itself: keeps what it has
    CHECK(c.p == bp && c.cap >= 64);
    touch(c);

    Buf d;
    CHECK(d.ensure(2000) == 0);
    void* dp = d.p;
    std::swap(c, d);
    CHECK(c.p == dp && d.p == bp && c.cap >= 2000 && d.cap >= 64 && Buf::live.load() == live0 + 2);
    touch(c), touch(d);
    Buf empty;
    std::swap(c, empty);  // with an empty one
    CHECK(c.p == nullptr && empty.p == dp);
  }
  CHECK(Buf::live.load() == live0);
}

// a struct with three buffers in a vector: grown by resize across two reallocations, then shrunk (Engine::clouds, the voxel slots, the keyframes)
struct Three {
  DevBuf a;
  PinnedBuf b;
  DevBuf c;
  int n = 0;
};
static void vector_of_owners() {
  std::vector<Three> v;
  v.resize(1);
  size_t reallocations = 0;
  for (size_t want : {2u, 3u, 5u, 9u, 17u}) {
    const Three* before = v.data();
    for (Three& t : v) {
      CHECK(t.a.ensure(48 + 16 * v.size()) == 0 && t.b.ensure(40) == 0 && t.c.ensure(8) == 0);
      t.n = (int)v.size();
    }
    v.resize(want);
    reallocations += v.data() != before;
    for (Three& t : v) touch(t.a), touch(t.b), touch(t.c);
  }
  CHECK(reallocations >= 2);
  CHECK(v[0].a.p && v[8].a.p && v[16].a.p == nullptr);
  CHECK(DevBuf::live.load() == 18 && PinnedBuf::live.load() == 9);
  v.resize(4);  // shrunk: the dropped elements free theirs
  CHECK(DevBuf::live.load() == 8 && PinnedBuf::live.load() == 4);
  std::swap(v[0], v[3]);
  touch(v[0].a), touch(v[3].a);
  v.erase(v.begin());  // (move assignment down the vector)
  CHECK(DevBuf::live.load() == 6 && PinnedBuf::live.load() == 3);
  for (Three& t : v) touch(t.a), touch(t.b), touch(t.c);
}

// the growth of the scan-context database (sc_reserve): four fresh buffers, the old contents copied, then fresh moved over old -- or an
// early return after two of the four, which must leave the old ones as they were and lose nothing
static int reserve_four(DevBuf (&db)[4], size_t bytes, long fail_after) {
  DevBuf* old[4] = {&db[0], &db[1], &db[2], &db[3]};
  DevBuf fresh[4];
  fake_fail_allocations_after(fail_after);
  for (int b = 0; b < 4; b++) APD_TRY(fresh[b].ensure(bytes));
  for (int b = 0; b < 4; b++)
    if (old[b]->p) std::memcpy(fresh[b].p, old[b]->p, old[b]->cap);
  for (int b = 0; b < 4; b++) *old[b] = std::move(fresh[b]);
  return 0;
}
static void array_of_four() {
  DevBuf db[4];
  CHECK(reserve_four(db, 256, -1) == 0);
  for (DevBuf& b : db) touch(b);
  CHECK(DevBuf::live.load() == 4);
  CHECK(reserve_four(db, 512, -1) == 0);  // replaced
  for (DevBuf& b : db) {
    CHECK(b.cap == 512);
    touch(b);
  }
  CHECK(DevBuf::live.load() == 4);
  void* kept[4] = {db[0].p, db[1].p, db[2].p, db[3].p};
  CHECK(reserve_four(db, 1024, 2) == APDGICP_ERR_HIP);  // the third allocation fails
  fake_fail_allocations_after(-1);
  CHECK(!g_last_error.empty());
  for (int b = 0; b < 4; b++) {
    CHECK(db[b].p == kept[b] && db[b].cap == 512);
    touch(db[b]);
  }
  CHECK(DevBuf::live.load() == 4);
  // a failed ensure of an owner leaves it empty, not dangling
  fake_fail_allocations_after(0);
  CHECK(db[0].ensure(4096) == APDGICP_ERR_HIP && db[0].p == nullptr && db[0].cap == 0);
  fake_fail_allocations_after(-1);
  CHECK(DevBuf::live.load() == 3);
}

static void cached_table() {
  hipStream_t st = nullptr;
  CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess);
  {
    CachedTable t;
    std::vector<int> small(8, 7), large(4000, 9);
    CHECK(t.upload(small.data(), small.size() * 4, st) == 0);
    CHECK(t.upload(small.data(), small.size() * 4, st) == 0);  // unchanged: no copy
    CHECK(hipStreamSynchronize(st) == hipSuccess);
    CHECK(t.dev.cap == 256 && std::memcmp(t.dev.p, small.data(), 32) == 0);
    CHECK(DevBuf::live.load() == 1 && PinnedBuf::live.load() == 1);
    CHECK(t.upload(large.data(), large.size() * 4, st) == 0);  // grows dev (and takes the other staging half)
    CHECK(hipStreamSynchronize(st) == hipSuccess);
    CHECK(t.dev.cap == 16128 && std::memcmp(t.dev.p, large.data(), 16000) == 0);
    CHECK(DevBuf::live.load() == 1 && PinnedBuf::live.load() == 2);
    large[17] = 1;
    CHECK(t.upload(large.data(), large.size() * 4, st) == 0);  // the first half again: grows it
    CHECK(hipStreamSynchronize(st) == hipSuccess);
    CHECK(t.as<int>()[17] == 1 && PinnedBuf::live.load() == 2);
    t.dev.release();  // (what apdgicp_batch_clear does to a mode's pair table) ... and the next upload brings it back
    CHECK(t.upload(large.data(), large.size() * 4, st) == 0);
    CHECK(hipStreamSynchronize(st) == hipSuccess);
    CHECK(t.as<int>()[17] == 1);
  }
  CHECK(hipStreamDestroy(st) == hipSuccess);
  CHECK(DevBuf::live.load() == 0 && PinnedBuf::live.load() == 0);
}

int main() {
  one_owner<DevBuf>(true);
  one_owner<PinnedBuf>(false);
  CHECK(fake_live_allocations() == 0);
  vector_of_owners();
  CHECK(fake_live_allocations() == 0);
  array_of_four();
  CHECK(fake_live_allocations() == 0);
  cached_table();
  const bool ok = g_bad == 0 && fake_live_allocations() == 0 && DevBuf::live.load() == 0 && PinnedBuf::live.load() == 0;
  std::printf("ok %d live_allocations %ld device %lld pinned %lld\n", ok ? 1 : 0, fake_live_allocations(), DevBuf::live.load(), PinnedBuf::live.load());
  return ok ? 0 : 1;
}
