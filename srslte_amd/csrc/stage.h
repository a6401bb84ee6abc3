// stage.h -- what a per-thread staging context is made of: its stream and its growable images.  What else a context holds (decoder and encoder objects,
// transform plans) and who owns it -- a StagePool (hip_common.h) for the contexts srsran_hip_warmup() prepares, thread_device_local for the rest -- is
// the business of the file that defines it.
#pragma once
#include "hip_common.h"

#include <cstring>
#include <map>
#include <utility>

namespace phyhip {

inline size_t al256(size_t v) // the next multiple of 256: the alignment of every region of a staging image
{
  return (v + 255) & ~(size_t)255;
}

// true when the n bytes at p (8-byte aligned, as the rows of a soft buffer are) are all zero: a row straight after srsran_softbuffer_rx_reset
// is not worth a copy, let alone a transfer.  Read-only, four independent accumulators (vectorises), early exit per 4 KB.
inline bool all_zero(const uint8_t* p, size_t n)
{
  size_t i = 0;
  if ((reinterpret_cast<uintptr_t>(p) & 7u) == 0) {
    const uint64_t* q = reinterpret_cast<const uint64_t*>(p);
    const size_t    w = n / 8;
    for (size_t j = 0; j < w;) {
      const size_t e = j + 512 < w ? j + 512 : w;
      uint64_t     a0 = 0, a1 = 0, a2 = 0, a3 = 0;
      for (; j + 4 <= e; j += 4) {
        a0 |= q[j], a1 |= q[j + 1], a2 |= q[j + 2], a3 |= q[j + 3];
      }
      for (; j < e; j++) {
        a0 |= q[j];
      }
      if (a0 | a1 | a2 | a3) {
        return false;
      }
    }
    i = w * 8;
  }
  for (; i < n; i++) {
    if (p[i]) {
      return false;
    }
  }
  return true;
}

// The context's stream: hipStreamNonBlocking, created by the first open() on the device the calling thread is bound to and destroyed with its owner.
// Creation is tried ONCE (device_available() is sticky: a later call would find what the first one found).  Converts to the stream it holds: nullptr
// until open() has succeeded, and always without a device.
class StageStream {
public:
  StageStream()                              = default;
  StageStream(const StageStream&)            = delete;
  StageStream& operator=(const StageStream&) = delete;
  ~StageStream()
  {
    if (st_) {
      (void)hipStreamDestroy(st_);
    }
  }
  bool open()
  {
    if (!tried_) {
      tried_ = true;
      if (device_available()) {
        bind_thread();
        if (hipStreamCreateWithFlags(&st_, hipStreamNonBlocking) != hipSuccess) {
          st_ = nullptr;
        }
      }
    }
    return st_ != nullptr;
  }
  operator hipStream_t() const { return st_; }

private:
  hipStream_t st_    = nullptr;
  bool        tried_ = false;
};

// A buffer of T that only grows: in device memory, as a pinned host image the kernels work on themselves (host_image_alloc), or in plain pinned memory
// (hipHostMalloc with default flags: the source and target of asynchronous copies).  grow(need) leaves a buffer that holds `need` elements alone; a
// smaller one is FREED and need + headroom elements are allocated -- the contents are not kept, and a failed allocation leaves nullptr and capacity 0.
// How much headroom a request gets is the site's policy (pinned memory is dear to re-allocate, and the first-call latencies on record were measured with
// these policies).  Converts to the pointer it holds.  Movable, so that its owners can live in containers and a grown table can take an old one's place.
enum class StageMem { Device, HostImage, Pinned };
template <StageMem M, class T = uint8_t>
class StageBuf {
public:
  StageBuf()                           = default;
  StageBuf(const StageBuf&)            = delete;
  StageBuf& operator=(const StageBuf&) = delete;
  StageBuf(StageBuf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr, o.cap_ = 0; }
  StageBuf& operator=(StageBuf&& o) noexcept
  {
    if (this != &o) {
      release();
      p_ = o.p_, cap_ = o.cap_;
      o.p_ = nullptr, o.cap_ = 0;
    }
    return *this;
  }
  ~StageBuf() { release(); }
  bool grow(size_t need, size_t headroom = 0) { return need <= cap_ || alloc(need + headroom); }
  bool alloc(size_t n) // a fresh buffer of exactly n elements, whatever was held
  {
    release();
    void*            p = nullptr;
    const hipError_t e = M == StageMem::Device ? hipMalloc(&p, n * sizeof(T)) : M == StageMem::HostImage ? host_image_alloc(&p, n * sizeof(T)) : hipHostMalloc(&p, n * sizeof(T));
    if (e != hipSuccess) {
      return false;
    }
    p_   = static_cast<T*>(p);
    cap_ = n;
    return true;
  }
  T*     get() const { return p_; }
  size_t cap() const { return cap_; } // elements
  operator T*() const { return p_; }
  T* operator->() const { return p_; }

private:
  void release()
  {
    if (p_) {
      (void)(M == StageMem::Device ? hipFree(p_) : hipHostFree(p_));
    }
    p_   = nullptr;
    cap_ = 0;
  }
  T*     p_   = nullptr;
  size_t cap_ = 0;
};
using DeviceBuf = StageBuf<StageMem::Device>;
using HostImage = StageBuf<StageMem::HostImage>;

// A device array and its host twin of the same layout (H: plain pinned memory for copies, or a host image the kernels read themselves), growing together by
// the site's headroom rule: the device side first, as every site allocated them.  After a failed grow() the side that failed is empty and the next call
// tries again.
template <class T = uint8_t, StageMem H = StageMem::Pinned, class TH = T> // (TH: the host's name for an element, where it has one of its own)
struct StagePair {
  static_assert(sizeof(T) == sizeof(TH), "one layout on both sides");
  StageBuf<StageMem::Device, T> d;
  StageBuf<H, TH>               h;
  bool grow(size_t need, size_t headroom = 0) { return d.grow(need, headroom) && h.grow(need, headroom); }
};

// a grow() result as what PHY_HIP_CHECK takes
inline hipError_t grown(bool ok)
{
  return ok ? hipSuccess : hipErrorOutOfMemory;
}

// "The previous call's kernel has consumed this buffer": an event recorded behind the launch and waited for before the host rewrites what the launch reads
// (and before its owner releases it).  Created with its owner; ok() tells whether that worked.
class StageEvent {
public:
  StageEvent()
  {
    if (hipEventCreateWithFlags(&ev_, hipEventDisableTiming) != hipSuccess) {
      ev_ = nullptr;
    }
  }
  StageEvent(const StageEvent&)            = delete;
  StageEvent& operator=(const StageEvent&) = delete;
  ~StageEvent()
  {
    if (ev_) {
      (void)hipEventDestroy(ev_);
    }
  }
  bool       ok() const { return ev_ != nullptr; }
  hipError_t wait() // for the recorded work, if any
  {
    if (!pending_) {
      return hipSuccess;
    }
    const hipError_t e = hipEventSynchronize(ev_);
    pending_           = e != hipSuccess;
    return e;
  }
  hipError_t record(hipStream_t st)
  {
    const hipError_t e = hipEventRecord(ev_, st);
    pending_           = pending_ || e == hipSuccess;
    return e;
  }

private:
  hipEvent_t ev_      = nullptr;
  bool       pending_ = false;
};

// A table of rows of `width` words on the device, one per key seen so far (CRC lane multipliers per message size).  With a pinned mirror, a new row is
// computed into the mirror by fill(row) and goes up by an asynchronous copy on the call's stream, in front of the kernel that reads it; without one it is
// computed on the stack and goes up with upload(), complete on return.  The table doubles when it is full and carries the old rows over; nothing may still
// read the old table or copy from the old mirror when they are released, hence the device-wide waits.  row() returns a row INDEX (the table may move while
// a call's jobs are still being written), or kNoRow with the error text set: "<who>: device allocation ..." or "<who>: upload ...".
class RowTable {
public:
  static constexpr uint32_t kNoRow = 0xffffffffu, kMaxWidth = 256; // (rows of 64 and of 256 lane multipliers exist)
  RowTable(uint32_t width, uint32_t first_cap, const char* who, bool mirror = true) : width_(width), first_cap_(first_cap), who_(who), mirror_(mirror) {}
  const uint32_t* device() const { return d_; }
  template <class Fill>
  uint32_t row(uint32_t key, hipStream_t st, Fill&& fill)
  {
    auto it = row_.find(key);
    if (it != row_.end()) {
      return it->second;
    }
    const uint32_t r = (uint32_t)row_.size();
    if (r >= rows_cap_) {
      const uint32_t                       cap = rows_cap_ ? 2 * rows_cap_ : first_cap_;
      StageBuf<StageMem::Device, uint32_t> nd;
      StageBuf<StageMem::Pinned, uint32_t> nh;
      if (!nd.grow((size_t)cap * width_) || (mirror_ && (!nh.grow((size_t)cap * width_) || hipDeviceSynchronize() != hipSuccess)) ||
          (d_ && (hipMemcpy(nd, d_, (size_t)r * width_ * sizeof(uint32_t), hipMemcpyDeviceToDevice) != hipSuccess || hipDeviceSynchronize() != hipSuccess))) {
        set_error("%s: device allocation of the CRC multiplier table failed", who_);
        return kNoRow;
      }
      if (h_) {
        memcpy(nh, h_, (size_t)r * width_ * sizeof(uint32_t));
      }
      d_        = std::move(nd);
      h_        = std::move(nh);
      rows_cap_ = cap;
    }
    uint32_t  tmp[kMaxWidth];
    uint32_t* m = mirror_ ? h_ + (size_t)r * width_ : tmp;
    fill(m);
    uint32_t* dst = d_ + (size_t)r * width_;
    if ((mirror_ ? hipMemcpyAsync(dst, m, width_ * sizeof(uint32_t), hipMemcpyHostToDevice, st) : upload(dst, m, width_ * sizeof(uint32_t))) != hipSuccess) {
      set_error("%s: upload of the CRC multiplier table failed", who_);
      return kNoRow;
    }
    row_.emplace(key, r);
    return r;
  }

private:
  std::map<uint32_t, uint32_t>         row_;
  StageBuf<StageMem::Device, uint32_t> d_;
  StageBuf<StageMem::Pinned, uint32_t> h_;
  uint32_t                             rows_cap_ = 0;
  const uint32_t                       width_, first_cap_;
  const char* const                    who_;
  const bool                           mirror_;
};

namespace rm {
bool build_all_tables(); // every rate-matching table in one allocation and one upload (rm_host.cpp): what srsran_hip_warmup (warmup_host.cpp) starts with
}

} // namespace phyhip
