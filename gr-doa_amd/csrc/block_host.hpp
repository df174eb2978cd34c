// block_host.hpp — host scaffold shared by the C entries of the blocks: the handle base, create and destroy, the argument
// checks, the host round trip of a `work` entry, and for the blocks that take or give N sample streams the stream checks,
// the input format, the window geometry and the staging of N streams.
// Host-only; nothing here launches a kernel.  INTEGRATION.md ("Adding a block") shows how an entry uses it.
#pragma once

#include <cstdint>
#include <initializer_list>

#include "common.hpp"

namespace doa {

// What every block's handle holds.  DevBuf / PinnedBuf / table members free themselves when the handle is deleted.
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

// N device streams of sb-byte samples: DOA_ERR_INVALID_ARG, with the error set, for a NULL stream or one not aligned to a
// sample (batch >= 0: named in the message).  *pair_aligned: every stream is aligned to two samples lead_bytes further on,
// where the kernel starts to read; the caller's route rule takes it from there.
inline int check_streams(const char *who, const void *const *d_in, int N, size_t sb, bool *pair_aligned, int batch = -1,
                         size_t lead_bytes = 0)
{
    *pair_aligned = true;
    char where[32] = "";
    if (batch >= 0) snprintf(where, sizeof where, " of batch %d", batch);
    for (int k = 0; k < N; k++) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(d_in[k]);
        if (!p) { set_error("%s: input stream %d%s is NULL", who, k, where); return DOA_ERR_INVALID_ARG; }
        if (p % sb) { set_error("%s: input stream %d%s is not %d-byte aligned", who, k, where, (int)sb); return DOA_ERR_INVALID_ARG; }
        if ((p + lead_bytes) % (2 * sb)) *pair_aligned = false;
    }
    return DOA_OK;
}

// The sample format of a stream-input block (doa_*_set_input_format): fc32, or sc16 widened as float(q) * scale.
struct InputFormat {
    int format = DOA_SAMPLE_FC32;
    float scale = 1.0f;
    int set(const char *who, int format_, float scale_)
    {
        if (const int rc = check_input_format(who, format_, scale_); rc != DOA_OK) return rc;
        format = format_; scale = scale_;
        return DOA_OK;
    }
    size_t sample_bytes() const { return doa::sample_bytes(format); }
    float kernel_scale() const { return format == DOA_SAMPLE_SC16 ? scale : 1.0f; }   // what a kernel multiplies by
};
// a doa_X_set_input_format entry (fmt: NULL for a NULL handle)
inline int set_input_format(const char *who, InputFormat *fmt, int format, float scale)
{
    if (fmt) return fmt->set(who, format, scale);
    set_error("%s_set_input_format: bad arguments", who);
    return DOA_ERR_INVALID_ARG;
}

// The window geometry of a block that cuts its streams into snapshots of K samples, `overlap` of them shared with the last.
struct StreamWindow {
    int K = 0, overlap = 0;
    int step() const { return K - overlap; }
    int history() const { return overlap + 1; }
    int forecast(int n) const { return step() * n; }
    long long input_span(int n) const { return n > 0 ? (long long)(n - 1) * step() + K : 0; }   // samples n items read
};

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
    // N host streams of `bytes` each, read from host[k] + src_off, go up into one buffer, stream_stride_bytes apart; d[k] is
    // stream k's device copy.  Every host pointer is checked before the first copy is queued.  keep_sample = 0: a copy starts
    // on its stride boundary whatever the host address.  keep_sample = the sample size: a copy keeps its host address modulo 16
    // (which must be aligned to one sample), so the load route a kernel picks from the alignment is the caller's own.
    int in_streams(const char *who, DevBuf &b, const void *const *host, int N, size_t bytes, const void **d, size_t src_off = 0,
                   size_t keep_sample = 0)
    {
        for (int k = 0; k < N && rc_ == DOA_OK; k++) {
            if (!host[k]) { set_error("%s: input_items[%d] is NULL", who, k); rc_ = DOA_ERR_INVALID_ARG; }
            else if (keep_sample && reinterpret_cast<uintptr_t>(host[k]) % keep_sample) {
                set_error("%s: input_items[%d] is not %d-byte aligned", who, k, (int)keep_sample);
                rc_ = DOA_ERR_INVALID_ARG;
            }
        }
        const size_t stride = stream_stride_bytes(bytes + (keep_sample ? 16 : 0));
        if (rc_ == DOA_OK) rc_ = b.reserve(stride * N);
        for (int k = 0; k < N && rc_ == DOA_OK; k++) {
            const char *src = static_cast<const char *>(host[k]) + src_off;
            char *dst = b.as<char>() + k * stride + (keep_sample ? reinterpret_cast<uintptr_t>(src) % 16 : 0);
            rc_ = hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st_), "the copy to the device");
            d[k] = dst;
        }
        return rc_;
    }
    // reserve now; finish() copies device -> host.  dst == nullptr (an absent optional output, or scratch): reserve only
    int out(DevBuf &b, void *dst, size_t bytes)
    {
        if (rc_ == DOA_OK) rc_ = b.reserve(bytes);
        if (rc_ == DOA_OK && dst) rc_ = pend(Pending{dst, nullptr, &b, bytes, 0, 0, 1});
        return rc_;
    }
    // N output streams of `bytes` each, `stride` bytes apart in one buffer (the block chooses the distance that keeps the
    // alignment its kernel wants); d[k] is where the device writes stream k, and finish() copies it to host[k] + dst_off.
    // Every host pointer is required.  The group is one pending entry, whatever N.
    int out_streams(const char *who, DevBuf &b, void *const *host, int N, size_t bytes, size_t stride, void **d, size_t dst_off = 0)
    {
        for (int k = 0; k < N && rc_ == DOA_OK; k++)
            if (!host[k]) { set_error("%s: output_items[%d] is NULL", who, k); rc_ = DOA_ERR_INVALID_ARG; }
        if (rc_ == DOA_OK) rc_ = b.reserve(stride * N);
        if (rc_ == DOA_OK) rc_ = pend(Pending{nullptr, host, &b, bytes, stride, dst_off, N});
        for (int k = 0; k < N && rc_ == DOA_OK; k++) d[k] = b.as<char>() + k * stride;
        return rc_;
    }
    // rc: what the entry's device step returned (>= 0: items done)
    int finish(int rc)
    {
        if (rc_ == DOA_OK && rc < 0) rc_ = rc;
        for (int i = 0; i < n_pending_; i++) {
            const Pending &p = pending_[i];
            for (int k = 0; k < p.n && rc_ == DOA_OK; k++) {
                void *dst = p.dsts ? static_cast<char *>(p.dsts[k]) + p.dst_off : p.dst;
                rc_ = hip(hipMemcpyAsync(dst, p.src->as<char>() + k * p.stride, p.bytes, hipMemcpyDeviceToHost, st_),
                          "the copy to the host");
            }
        }
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
    // one buffer (dst) or a group of n streams (dsts[k] + dst_off), `stride` apart on the device
    struct Pending { void *dst; void *const *dsts; const DevBuf *src; size_t bytes, stride, dst_off; int n; };
    int pend(const Pending &p)
    {
        if (n_pending_ < kMaxPending) { pending_[n_pending_++] = p; return DOA_OK; }
        set_error("HostCall: more than %d outputs", kMaxPending);
        return DOA_ERR_INVALID_ARG;
    }
    hipStream_t st_;
    int rc_;
    Pending pending_[kMaxPending];
    int n_pending_ = 0;
};

}  // namespace doa
