// One synchronous, host-buffer call on device 0 (DESIGN.md "Staged calls"):
// the inputs are gathered in a pinned buffer at the offsets of a StageLayout
// (host/stage_layout.h), copied to the device in one piece, the launches run,
// and the outputs come back in one piece.  A new synchronous entry point
// starts here.  Included by tmverify_runtime.cpp, whose Device, bounded waits
// and error text it uses.  The steps, each returning 0 or the entry point's
// return code with the error text set:
//   attach   the context: TMV_ERR_ARG for none
//   open     takes the device's lock -- held until the object goes, so until
//            the last byte has left the pinned buffer -- and waits for the
//            context stream, which an earlier device-pointer call may still
//            have reading these buffers
//   reserve  the pinned and the device buffer; via_pinned: the outputs come
//            back through the pinned buffer (finish without a destination)
//   put      inputs into the pinned buffer
//   upload   the one copy to the device
//   finish   the one copy back (to dst, else to the pinned buffer) and the wait
#pragma once
#include "host/stage_layout.h"

namespace {

struct StagedCall {
  Device *d = nullptr;
  std::unique_lock<std::mutex> lk;
  hipStream_t s = nullptr;
  const tmh::StageLayout *L = nullptr;
  uint8_t *h = nullptr, *g = nullptr;  // the pinned and the device buffer

  int attach(tmv_ctx *ctx) {
    if (!ctx || ctx->devs.empty()) { set_error("null context"); return TMV_ERR_ARG; }
    d = ctx->devs[0].get();
    return 0;
  }
  int open() {
    lk = std::unique_lock<std::mutex>(d->mu);
    if (d->faulted) return faulted_rc(*d);
    const int rc = use_device(*d, nullptr, &s);
    if (rc != 0) return rc;
    const hipError_t e = wait_stream(*d, s);
    return e != hipSuccess ? wait_rc(e) : 0;
  }
  int reserve(const tmh::StageLayout &layout, DeviceBuf &hb, DeviceBuf &db, bool via_pinned) {
    L = &layout;
    hipError_t e = hb.ensure(via_pinned ? std::max(L->in_bytes, L->out_bytes) : L->in_bytes, true);
    if (e != hipSuccess) { set_error("hipHostMalloc", e); return TMV_ERR_NOMEM; }
    if ((e = db.ensure(L->dev_bytes, false)) != hipSuccess) { set_error("hipMalloc", e); return TMV_ERR_NOMEM; }
    h = static_cast<uint8_t *>(hb.ptr);
    g = static_cast<uint8_t *>(db.ptr);
    if (L->pad_at) std::memset(h + L->pad_at - 16, 0, 16);
    return 0;
  }
  void put(size_t at, const void *src, size_t bytes) {
    if (bytes) std::memcpy(h + at, src, bytes);
  }
  int upload(const char *what) {  // what: "hipMemcpyAsync(<call>)"
    const hipError_t e = hipMemcpyAsync(g, h, L->in_bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) { set_error(what, e); return TMV_ERR_LAUNCH; }
    return 0;
  }
  template <class T>
  T *dev(size_t at) const { return reinterpret_cast<T *>(g + at); }
  // what: "<call> readback".  A timed-out wait has set its own text.
  int finish(const char *what, void *dst = nullptr, size_t bytes = 0) {
    hipError_t e = hipMemcpyAsync(dst ? dst : h, g + L->out_at, dst ? bytes : L->out_bytes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess || (e = wait_stream(*d, s)) != hipSuccess) {
      if (e != hipErrorNotReady) set_error(what, e);
      return wait_rc(e);
    }
    return 0;
  }
  // After finish(): an output region in the pinned buffer.
  const uint8_t *result(size_t at) const { return h + (at - L->out_at); }
};

// 0, or TMV_ERR_ARG and "<fn>: <name>[0] must be 0" / "<fn>: <name> decreasing".
int offsets_rc(const char *fn, const char *name, const uint32_t *off, uint32_t n, uint32_t *max_span = nullptr) {
  const tmh::Offsets r = tmh::check_offsets(off, n, max_span);
  if (r == tmh::Offsets::kOk) return 0;
  set_error(std::string(fn) + ": " + name + (r == tmh::Offsets::kDecreasing ? " decreasing" : "[0] must be 0"));
  return TMV_ERR_ARG;
}

}  // namespace
