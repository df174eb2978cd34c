// block_host.hpp — host scaffold shared by the C entries of the blocks that take one item stream (covariance items or
// spectra): the handle base, create and destroy, the argument checks, and the host round trip of a `work` entry.
// Host-only; nothing here launches a kernel.  INTEGRATION.md ("Adding a block") shows how an entry uses it.
#pragma once

#include <initializer_list>

#include "common.hpp"

namespace doa {

// What every item block's handle holds.  DevBuf / PinnedBuf / table members free themselves when the handle is deleted.
struct BlockBase {
    int bits = 64;                // internal precision: the process default at create (doa_set_internal_precision)
    int device = 0;               // the device the handle was created on
    long long items_total = 0;
    hipStream_t stream = nullptr; // the host entries' own stream
};

template <class H> void destroy_block(H *h)
{
    if (!h) return;
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

// The tail of every create, run after the caller's argument validation (arguments are refused before the device is looked
// for): device, handle, stream, then init(*h) -> DOA_OK or an error (the block's parameters and table build).
template <class H, class Init> H *create_block(const char *who, Init &&init)
{
    int dev = 0;
    if (ensure_device(&dev) != DOA_OK) return nullptr;
    H *h = new (std::nothrow) H();
    if (!h) { set_error("%s: out of memory", who); return nullptr; }
    h->device = dev;
    h->bits = internal_precision_bits();
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess || init(*h) != DOA_OK) {
        if (!*doa_last_error()) set_error("%s: device setup failed", who);
        destroy_block(h);
        return nullptr;
    }
    return h;
}

// DOA_ERR_INVALID_ARG unless there is a handle, n >= min_n and, for n > 0, every required pointer.
inline int work_args(const char *who, const void *h, int n, std::initializer_list<const void *> required, int min_n = 0)
{
    bool ok = h && n >= min_n;
    if (ok && n > 0) for (const void *p : required) ok = ok && p;
    if (!ok) set_error("%s: bad arguments (NULL handle or required pointer, or fewer than %d items: %d)", who, min_n, n);
    return ok ? DOA_OK : DOA_ERR_INVALID_ARG;
}

inline int need_bits64(const char *who, int bits, const char *what)
{
    if (bits == 64) return DOA_OK;
    set_error("%s: %s needs internal precision 64 (handle is at %d)", who, what, bits);
    return DOA_ERR_UNSUPPORTED;
}

// The host round trip of one entry on the handle's stream: in() buffers go up, the entry queues its device work, finish()
// brings the out() buffers down.  Whatever fails, finish() returns with the stream synchronised, so no copy that reads or
// writes the caller's memory is in flight after the entry has returned.  The first failure sticks; later calls do nothing.
class HostCall {
public:
    explicit HostCall(const BlockBase &b) : st_(b.stream), rc_(bind_device(b.device)) {}
    HostCall(const HostCall &) = delete;
    HostCall &operator=(const HostCall &) = delete;

    int status() const { return rc_; }
    // reserve + copy host -> device
    int in(DevBuf &b, const void *src, size_t bytes)
    {
        if (rc_ == DOA_OK) rc_ = b.reserve(bytes);
        if (rc_ == DOA_OK) rc_ = hip(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st_), "the copy to the device");
        return rc_;
    }
    // reserve now; finish() copies device -> host.  dst == nullptr (an absent optional output, or scratch): reserve only
    int out(DevBuf &b, void *dst, size_t bytes)
    {
        if (rc_ == DOA_OK) rc_ = b.reserve(bytes);
        if (rc_ == DOA_OK && dst) {
            if (n_pending_ < kMaxPending) pending_[n_pending_++] = Pending{dst, &b, bytes};
            else { set_error("HostCall: more than %d outputs", kMaxPending); rc_ = DOA_ERR_INVALID_ARG; }
        }
        return rc_;
    }
    // rc: what the entry's device step returned (>= 0: items done)
    int finish(int rc)
    {
        if (rc_ == DOA_OK && rc < 0) rc_ = rc;
        for (int i = 0; i < n_pending_ && rc_ == DOA_OK; i++)
            rc_ = hip(hipMemcpyAsync(pending_[i].dst, pending_[i].src->p, pending_[i].bytes, hipMemcpyDeviceToHost, st_),
                      "the copy to the host");
        const hipError_t e = hipStreamSynchronize(st_);
        if (rc_ == DOA_OK) rc_ = hip(e, "hipStreamSynchronize");
        return rc_ == DOA_OK ? rc : rc_;
    }

private:
    static int hip(hipError_t e, const char *what)
    {
        if (e == hipSuccess) return DOA_OK;
        set_error("%s failed: %s", what, hipGetErrorString(e));
        return (e == hipErrorNoDevice || e == hipErrorInvalidDevice) ? DOA_ERR_NO_DEVICE : DOA_ERR_HIP;
    }
    static constexpr int kMaxPending = 4;
    struct Pending { void *dst; const DevBuf *src; size_t bytes; };
    hipStream_t st_;
    int rc_;
    Pending pending_[kMaxPending];
    int n_pending_ = 0;
};

}  // namespace doa
