/*
 * ssd_owned.h — the four HIP resources the host code holds, each in a move-only owner: device memory, pinned host memory, an event,
 * a stream.  An owner is empty by default, cannot be copied (its move operations take that away), frees what it holds in its destructor,
 * and converts to the raw pointer or handle (get(), or implicitly: an inline load), so that launchers and HIP calls take it as they took
 * the raw field.  Host only.
 *
 * An acquiring call returns the hipError_t; on failure the owner is empty and HIP's error state is cleared (the failure is the
 * caller's to report, not a later HIP_TRY's).
 *
 * All-or-nothing groups: acquire every member into LOCALS; only when the last one has succeeded, std::move them into the handle.  A
 * failure in between returns, the locals' destructors free what was made, and the handle is as it was:
 *
 *     DeviceBuf<T> d;  PinnedBuf<T> p;  Event copied;
 *     hipError_t e = d.alloc(bytes, &h->bytes);
 *     if(e == hipSuccess) e = p.alloc(bytes);
 *     if(e == hipSuccess) e = copied.create(hipEventDisableTiming);
 *     if(e != hipSuccess) return fail(hip_error_code(e), ...);
 *     h->dThing = std::move(d);  h->hThing = std::move(p);  h->thingCopied = std::move(copied);
 *
 * Accounting: a buffer allocated with a ledger (ssd_handle::bytes) adds its size there when it is made and takes it back when it is
 * reset or destroyed, wherever it has been moved in between; one allocated without is not counted.  The ledger must outlive the
 * buffer (the handle's own field does: its buffers are its members).
 */
#ifndef SSD_OWNED_H_
#define SSD_OWNED_H_

#include "../../include/ssd_hip.h"
#include <hip/hip_runtime.h>
#include <cstddef>
#include <utility>
#include <vector>

namespace ssd
{

/* SSD_E_NOMEM for an allocation that did not fit, SSD_E_HIP for every other failure; the caller adds its message */
inline int hip_error_code(hipError_t e) { return e == hipErrorOutOfMemory ? SSD_E_NOMEM : SSD_E_HIP; }

/* what the two kinds of memory differ in */
struct DeviceMem
{
  static hipError_t make(void **p, size_t bytes) { return hipMalloc(p, bytes); }
  static void drop(void *p) { (void)hipFree(p); }
};
struct PinnedMem
{
  static hipError_t make(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void drop(void *p) { (void)hipHostFree(p); }
};

template<typename T, typename Mem>
class Buf
{
public:
  Buf() = default;
  explicit Buf(T *released) : p_(released) {}      /* takes back what release() gave away (not counted) */
  Buf(Buf &&o) noexcept : p_(o.p_), counted_(o.counted_), ledger_(o.ledger_) { o.forget(); }
  Buf &operator=(Buf &&o) noexcept
  {
    if(this != &o)
    {
      reset();
      p_ = o.p_; counted_ = o.counted_; ledger_ = o.ledger_;
      o.forget();
    }
    return *this;
  }
  ~Buf() { reset(); }

  /* `bytes` of memory in place of what the owner held; counted in *ledger (if any) for as long as the owner holds it */
  hipError_t alloc(size_t bytes, size_t *ledger = nullptr)
  {
    reset();
    void *p = nullptr;
    const hipError_t e = Mem::make(&p, bytes);
    if(e != hipSuccess)
    {
      (void)hipGetLastError();
      return e;
    }
    p_ = static_cast<T *>(p);
    ledger_ = ledger;
    counted_ = ledger ? bytes : 0;
    if(ledger_) *ledger_ += counted_;
    return hipSuccess;
  }
  void reset()
  {
    if(p_) Mem::drop(p_);
    if(ledger_) *ledger_ -= counted_;
    forget();
  }
  /* the memory is the caller's to free from here on; what it counted stays counted (it is still allocated) */
  T *release() { T *p = p_; forget(); return p; }
  T *get() const { return p_; }
  operator T *() const { return p_; }

private:
  void forget() { p_ = nullptr; counted_ = 0; ledger_ = nullptr; }
  T *p_ = nullptr;
  size_t counted_ = 0;
  size_t *ledger_ = nullptr;
};

template<typename T> using DeviceBuf = Buf<T, DeviceMem>;
template<typename T> using PinnedBuf = Buf<T, PinnedMem>;

/* the two kinds of handle: Raw is a pointer type of HIP's */
template<typename Raw, hipError_t (*Make)(Raw *, unsigned int), hipError_t (*Drop)(Raw)>
class Owned
{
public:
  Owned() = default;
  Owned(Owned &&o) noexcept : r_(o.release()) {}
  Owned &operator=(Owned &&o) noexcept
  {
    if(this != &o)
    {
      reset();
      r_ = o.release();
    }
    return *this;
  }
  ~Owned() { reset(); }

  /* flags: hipEventDefault for an event that is timed, hipEventDisableTiming for one that only orders; hipStreamNonBlocking */
  hipError_t create(unsigned int flags)
  {
    reset();
    const hipError_t e = Make(&r_, flags);
    if(e != hipSuccess)
    {
      r_ = nullptr;
      (void)hipGetLastError();
    }
    return e;
  }
  void reset()
  {
    if(r_) (void)Drop(r_);
    r_ = nullptr;
  }
  Raw release() { Raw r = r_; r_ = nullptr; return r; }
  Raw get() const { return r_; }
  operator Raw() const { return r_; }

private:
  Raw r_ = nullptr;
};

using Event = Owned<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

/* n events with the same flags, or none: `out` is replaced only when all of them were made */
inline hipError_t make_events(std::vector<Event> &out, size_t n, unsigned int flags)
{
  std::vector<Event> ev(n);
  for(Event &e : ev)
    if(const hipError_t rc = e.create(flags); rc != hipSuccess)
      return rc;
  out.swap(ev);
  return hipSuccess;
}

} // namespace ssd

#endif /* SSD_OWNED_H_ */
