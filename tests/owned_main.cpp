/*
 * owned_main.cpp — the owners of csrc/ssd_owned.h by themselves (tests/test_owned.py builds and runs this program).
 *
 * Without a HIP device every acquisition fails ("no device"), so the failure semantics run as they are; an allocation of
 * 2^62 bytes fails with a device too.  Where a device exists the successful paths run as well.  Exit status 0 = every check held.
 */
#include "ssd_owned.h"

#include <cstdio>
#include <utility>

using namespace ssd;

static int g_failed = 0;
#define CHECK(cond)                                                                  \
  do                                                                                 \
  {                                                                                  \
    if(!(cond))                                                                      \
    {                                                                                \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);                  \
      g_failed++;                                                                    \
    }                                                                                \
  } while(0)

static const size_t kTooMuch = size_t(1) << 62;

/* what a handle's feature looks like: three resources and the ledger they are counted in */
struct Target
{
  DeviceBuf<int> d;
  PinnedBuf<int> p;
  Event ev;
  size_t bytes = 0;
};

/* the all-or-nothing idiom of ssd_owned.h, with a last member of lastBytes */
static hipError_t make_group(Target &t, size_t lastBytes)
{
  DeviceBuf<int> d;
  PinnedBuf<int> p;
  Event ev;
  DeviceBuf<char> last;
  hipError_t e = d.alloc(256, &t.bytes);
  if(e == hipSuccess) e = p.alloc(256, &t.bytes);
  if(e == hipSuccess) e = ev.create(hipEventDisableTiming);
  if(e == hipSuccess) e = last.alloc(lastBytes, &t.bytes);
  if(e != hipSuccess)
    return e;
  t.d = std::move(d); t.p = std::move(p); t.ev = std::move(ev);
  return hipSuccess;                                /* `last` goes with the call: its share leaves the ledger again */
}

/* HIP keeps the last error per thread; without a device the query itself fails ("no device"), so there is nothing to ask */
static bool g_device = false;
static bool error_state_clear()
{
  return !g_device || hipGetLastError() == hipSuccess;
}

int main()
{
  int nDev = 0;
  const bool device = g_device = hipGetDeviceCount(&nDev) == hipSuccess && nDev > 0;
  (void)hipGetLastError();

  /* the error mapping */
  CHECK(hip_error_code(hipErrorOutOfMemory) == SSD_E_NOMEM);
  CHECK(hip_error_code(hipErrorInvalidValue) == SSD_E_HIP);
  CHECK(hip_error_code(hipErrorNoDevice) == SSD_E_HIP);

  /* empty by default; reset() and release() of an empty owner change nothing */
  {
    DeviceBuf<int> d;
    PinnedBuf<float> p;
    Event ev;
    Stream s;
    CHECK(!d && !p && !ev && !s && d.get() == nullptr && ev.get() == nullptr);
    d.reset(); p.reset(); ev.reset(); s.reset();
    CHECK(d.release() == nullptr && p.release() == nullptr && ev.release() == nullptr && s.release() == nullptr);
    CHECK(!d && !p && !ev && !s);
  }

  /* a failed acquire returns the error, leaves the owner empty, the ledger as it was and HIP's error state clear */
  {
    size_t ledger = 77;
    DeviceBuf<int> d;
    PinnedBuf<int> p;
    CHECK(d.alloc(kTooMuch, &ledger) != hipSuccess && !d);
    CHECK(error_state_clear());
    CHECK(p.alloc(kTooMuch, &ledger) != hipSuccess && !p);
    CHECK(error_state_clear());
    CHECK(ledger == 77);
    Event ev;
    Stream s;
    const hipError_t ee = ev.create(hipEventDisableTiming), es = s.create(hipStreamNonBlocking);
    CHECK((ee == hipSuccess) == (ev.get() != nullptr) && (es == hipSuccess) == (s.get() != nullptr));
    CHECK((ee == hipSuccess) == device && (es == hipSuccess) == device);
    CHECK(error_state_clear());
    std::vector<Event> evs;
    const hipError_t en = make_events(evs, 6, hipEventDefault);
    CHECK(en == hipSuccess ? evs.size() == 6 && evs[5].get() != nullptr : evs.empty());
  }

  /* moves leave the source empty (an adopted address that is never freed: release() takes it back before the owner ends) */
  {
    int x = 0;
    DeviceBuf<int> a(&x);
    DeviceBuf<int> b(std::move(a));
    CHECK(!a && b.get() == &x);
    DeviceBuf<int> c;
    c = std::move(b);
    CHECK(!b && c.get() == &x && static_cast<int *>(c) == &x);
    CHECK(c.release() == &x && !c);
  }

  /* a group whose last member cannot be had leaves an empty target empty ... */
  {
    Target t;
    t.bytes = 1000;
    CHECK(make_group(t, kTooMuch) != hipSuccess);
    CHECK(!t.d && !t.p && !t.ev && t.bytes == 1000);
    CHECK(error_state_clear());
    /* ... and a filled one as it was (filled only where there is a device to fill it from) */
    const hipError_t e = make_group(t, 16);
    CHECK((e == hipSuccess) == device);
    if(e == hipSuccess)
    {
      int *const d = t.d.get(), *const p = t.p.get();
      const hipEvent_t ev = t.ev.get();
      CHECK(d && p && ev && t.bytes == 1000 + 512);
      CHECK(make_group(t, kTooMuch) != hipSuccess);
      CHECK(t.d.get() == d && t.p.get() == p && t.ev.get() == ev && t.bytes == 1000 + 512);
      /* the share travels with the buffer and leaves with it */
      DeviceBuf<int> moved(std::move(t.d));
      CHECK(!t.d && moved.get() == d && t.bytes == 1000 + 512);
      moved.reset();
      CHECK(t.bytes == 1000 + 256);
      Event ev2(std::move(t.ev));
      CHECK(!t.ev && ev2.get() == ev);
      t.p.reset();
      CHECK(!t.p && t.bytes == 1000);
    }
  }

  if(g_failed)
    return 1;
  std::printf("owned: ok (%s)\n", device ? "with a device" : "no device: failure paths only");
  return 0;
}
