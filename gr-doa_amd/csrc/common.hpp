// common.hpp — shared host-side plumbing of libdoa_hip.so (error reporting, HIP call checks,
// small device-buffer helper, the wave size and the non-temporal 16-byte accesses).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>

#include "../../include/doa_hip.h"
#include "../../include/doa_hip_test.h"

namespace doa {

// ---- error reporting ------------------------------------------------------------------------
void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
void clear_error();

#define DOA_HIP_TRY(expr)                                                                       \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) {                                                                 \
            ::doa::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,   \
                             __LINE__);                                                         \
            return (_e == hipErrorNoDevice || _e == hipErrorInvalidDevice) ? DOA_ERR_NO_DEVICE  \
                                                                           : DOA_ERR_HIP;       \
        }                                                                                       \
    } while (0)

// Binds the calling thread to a usable HIP device (the current one); DOA_ERR_NO_DEVICE if none.  First call per device: populates
// the runtime's hardware-queue pool (prime_hw_queues, common.hip).
int ensure_device(int *device_out);
// Makes `device` (the one the handle was created on) current for the calling thread if it is not.
int bind_device(int device);
// Compute units of the current device (cached); the grid caps of the streaming kernels are multiples of it.
int cu_count();

// ---- grow-only device / pinned-host buffers ----------------------------------------------------
// Each owns its allocation: freed by release() (idempotent) or with the object; movable, not copyable.
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    int reserve(size_t bytes);  // DOA_OK or error; keeps contents only if no growth was needed
    void release();
    template <class T> T *as() const { return static_cast<T *>(p); }
};
struct PinnedBuf {
    void *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(PinnedBuf &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    PinnedBuf &operator=(PinnedBuf &&o) noexcept
    {
        if (this != &o) { release(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
        return *this;
    }
    ~PinnedBuf() { release(); }
    int reserve(size_t bytes);
    void release();
    template <class T> T *as() const { return static_cast<T *>(p); }
};

int internal_precision_bits();  // 32 or 64 (doa_set_internal_precision)

// the input sample formats (DOA_SAMPLE_FC32 / DOA_SAMPLE_SC16): bytes per sample, and the validation behind every
// doa_*_set_input_format entry (DOA_OK, or DOA_ERR_INVALID_ARG with the error set)
inline size_t sample_bytes(int format) { return format == DOA_SAMPLE_SC16 ? 4 : 8; }
int check_input_format(const char *what, int format, float scale);

// Launch-shape knobs for same-box A/B runs exist only in lab builds (make LAB=1); the default build has none of them
// compiled in and this is the constant `dflt`.
#ifdef DOA_LAB
#define DOA_LAB_ENV_INT(name, dflt) ([] { static const int v_ = [] { const char *e_ = getenv(name); return e_ ? atoi(e_) : (dflt); }(); return v_; }())
#else
#define DOA_LAB_ENV_INT(name, dflt) (dflt)
#endif

// Distance between the device copies of consecutive input streams (doa_stream_stride_bytes): the stream size rounded up
// to 8 KiB plus 4.5 KiB, so that stream k starts 4.5 k KiB further into the 8 KiB period than stream 0 -- sixteen
// distinct multiples of 512 B for sixteen streams (9 is odd).  See include/doa_hip.h for the measurement.
inline size_t stream_stride_bytes(size_t stream_bytes) { return ((stream_bytes + 8191) & ~(size_t)8191) + 4608; }

// ---- a wave = 64 lanes on gfx950; the moves and reductions between them are in wave_ops.hpp ----
constexpr int kWave = 64;

// streamed-once data: non-temporal 16-byte accesses (read-once input samples, write-once spectra)
typedef float doa_f32x4 __attribute__((ext_vector_type(4)));
template <bool NT> __device__ __forceinline__ float4 load_f4(const float4 *p)
{
    if constexpr (NT) {
        const doa_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const doa_f32x4 *>(p));
        return make_float4(v.x, v.y, v.z, v.w);
    } else {
        return *p;
    }
}
template <bool NT> __device__ __forceinline__ void store_f4(float4 *p, float4 v)
{
    if constexpr (NT) {
        doa_f32x4 t = {v.x, v.y, v.z, v.w};
        __builtin_nontemporal_store(t, reinterpret_cast<doa_f32x4 *>(p));
    } else {
        *p = v;
    }
}

}  // namespace doa
