// rust-modem_amd/csrc/capi_common.h — what every host unit of the C ABI (csrc/capi_*.cpp, the
// implementation of include/modem_hip.h) shares: device selection, device allocations, pointer
// classification and the one host / device I/O path of the process() calls. Not part of the ABI.
// The units that evaluate host floating point state `#pragma clang fp contract(off)` themselves,
// so that their float expressions round like rustc's.
#pragma once
#include "../../include/modem_hip.h"
#include "modem_internal.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <memory>
#include <new>
#include <vector>

namespace capi {

constexpr float kPi = 3.14159265358979323846f;   // std::f32::consts::PI

struct DeviceGuard {   // scoped hipSetDevice (no call when the device is already current)
    int old = -1;
    bool ok = false, set = false;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&old) != hipSuccess) { (void)hipGetLastError(); old = -1; }
        if (old == dev) { ok = true; return; }
        ok = hipSetDevice(dev) == hipSuccess;
        set = ok;
        if (!ok) (void)hipGetLastError();
    }
    ~DeviceGuard() { if (set && old >= 0) (void)hipSetDevice(old); }
};

// The one attribute query of a user pointer (the per-call host cost of a process() is mostly these
// queries): host memory (staged), device memory the handle's kernels can use (managed memory
// counts as the handle's device), or another GPU's memory (refused: it would be read over the
// fabric or fault; the reference has one address space, no counterpart). NULL is not queried.
enum PtrKind { PTR_HOST = 0, PTR_DEVICE = 1, PTR_FOREIGN = 2 };
inline PtrKind ptr_kind(const void* p, int dev) {
    if (!p) return PTR_HOST;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return PTR_HOST; }
    if (a.type == hipMemoryTypeManaged) return PTR_DEVICE;
    if (a.type != hipMemoryTypeDevice) return PTR_HOST;
    return a.device == dev ? PTR_DEVICE : PTR_FOREIGN;
}

#define HIP_TRY(expr)                                                              \
    do {                                                                           \
        if ((expr) != hipSuccess) { (void)hipGetLastError(); return MODEM_ERR_HIP; } \
    } while (0)

template <typename T>
modem_status dalloc(T** p, size_t count) {
    *p = nullptr;
    if (count == 0) count = 1;
    if (hipMalloc(reinterpret_cast<void**>(p), count * sizeof(T)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return MODEM_ERR_ALLOC;
    }
    if (hipMemset(*p, 0, count * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return MODEM_ERR_HIP; }
    return MODEM_OK;
}

// `count` elements of T from host memory into device memory (a *_create's tables; synchronous).
template <typename T>
modem_status h2d(T* dst, const void* src, size_t count) {
    HIP_TRY(hipMemcpy(dst, src, count * sizeof(T), hipMemcpyHostToDevice));
    return MODEM_OK;
}
// The same into a new allocation.
template <typename T>
modem_status upload(T** dst, const void* src, size_t count) {
    const modem_status st = dalloc(dst, count);
    return st ? st : h2d(*dst, src, count);
}

// Growable device staging buffer for host-pointer I/O.
struct Stage {
    void* p = nullptr;
    size_t cap = 0;
    modem_status ensure(size_t bytes) {
        if (bytes <= cap) return MODEM_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return MODEM_ERR_ALLOC; }
        cap = bytes;
        return MODEM_OK;
    }
    ~Stage() { if (p) (void)hipFree(p); }
};

// Growable device workspace of a handle's device-only path (include/modem_hip.h, "Streams").
// Growing never frees: hipFree waits for the whole device, which a call documented as asynchronous
// must not do, and kernels already queued may still use the old buffer. A buffer that was outgrown
// is retired and lives until the handle is destroyed; the capacity at least doubles each time, so
// the retired buffers together stay below the live one.
struct Workspace {
    void* p = nullptr;
    size_t cap = 0;
    std::vector<void*> retired;
    modem_status ensure(size_t bytes) {
        if (bytes <= cap) return MODEM_OK;
        const size_t want = std::max(bytes, 2 * cap);
        void* q = nullptr;
        if (hipMalloc(&q, want) != hipSuccess) { (void)hipGetLastError(); return MODEM_ERR_ALLOC; }
        if (p) retired.push_back(p);
        p = q;
        cap = want;
        return MODEM_OK;
    }
    ~Workspace() {
        if (p) (void)hipFree(p);
        for (void* r : retired) (void)hipFree(r);
    }
};

inline bool device_ok(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return false; }
    return device >= 0 && device < n;
}

// The prologue of a *_create: the device exists and is current for the rest of the scope, and `h`
// is a new handle on it, deleted by every return until h.release() hands it to the caller.
#define NEW_HANDLE(T, h, dev)                                \
    if (!device_ok(dev)) return MODEM_ERR_NO_DEVICE;         \
    DeviceGuard h##_guard(dev);                              \
    if (!h##_guard.ok) return MODEM_ERR_NO_DEVICE;           \
    std::unique_ptr<T> h(new (std::nothrow) T);              \
    if (!h) return MODEM_ERR_ALLOC;                          \
    h->device = dev

// Bytes of one scalar of a MODEM_DTYPE_* code (an I/Q pair is two of them).
inline size_t dtype_bytes(int32_t dt) { return dt == MODEM_DTYPE_F32 ? 4 : dt == MODEM_DTYPE_I8 ? 1 : 2; }
inline bool llr_dtype_ok(int32_t dt) { return dt == MODEM_DTYPE_F32 || dt == MODEM_DTYPE_F16 || dt == MODEM_DTYPE_I8; }
inline bool iq_dtype_ok(int32_t dt) { return dt == MODEM_DTYPE_F32 || dt == MODEM_DTYPE_F16; }

// One user pointer of a call. Until HostIo::take classifies it, it counts as device memory that the
// kernel uses as it is: what a NULL pointer and the pointer of an empty buffer stay.
struct IoPtr {
    void* user;
    void* dev;                   // what the kernel gets: `user`, or the stage once in() / out() staged it
    PtrKind kind = PTR_DEVICE;
    IoPtr(const void* p = nullptr) : user(const_cast<void*>(p)), dev(user) {}
    bool staged() const { return dev != user; }
    template <typename T> T* as() const { return static_cast<T*>(dev); }
};

// Host / device I/O of one call: take() classifies each user pointer once, and that one answer
// decides the refusal, the staging (inputs before the launch, outputs copied back after it), the
// buffer the kernel gets, and whether the call synchronises the stream before it returns (if and
// only if a host buffer was staged in or copied back).
struct HostIo {
    int device;
    hipStream_t s;
    bool sync = false;
    // False: the call refuses the pointer — memory of another GPU, a device pointer that is not a
    // multiple of `align` (0: any), or with `device_only` anything but the device's memory.
    bool take(IoPtr& io, size_t align = 0, bool device_only = false) const {
        if (!io.user) return true;
        io.kind = ptr_kind(io.user, device);
        if (io.kind == PTR_DEVICE) return !align || reinterpret_cast<uintptr_t>(io.user) % align == 0;
        return io.kind == PTR_HOST && !device_only;
    }
    modem_status in(IoPtr& io, Stage& st, size_t bytes) {
        if (io.kind != PTR_HOST || !bytes) return MODEM_OK;
        modem_status e;
        if ((e = st.ensure(bytes))) return e;
        HIP_TRY(hipMemcpyAsync(st.p, io.user, bytes, hipMemcpyHostToDevice, s));
        io.dev = st.p;
        sync = true;
        return MODEM_OK;
    }
    modem_status out(IoPtr& io, Stage& st, size_t bytes) {
        if (io.kind != PTR_HOST || !bytes) return MODEM_OK;
        modem_status e;
        if ((e = st.ensure(bytes))) return e;
        io.dev = st.p;
        return MODEM_OK;
    }
    modem_status back(const IoPtr& io, size_t bytes) {          // after the launch
        if (!io.staged() || !bytes) return MODEM_OK;
        HIP_TRY(hipMemcpyAsync(io.user, io.dev, bytes, hipMemcpyDeviceToHost, s));
        sync = true;
        return MODEM_OK;
    }
    // Device data of the call (not a staged copy of the buffer) to a user pointer on either side.
    modem_status put(const IoPtr& io, const void* src, size_t bytes) {
        HIP_TRY(hipMemcpyAsync(io.user, src, bytes, hipMemcpyDefault, s));
        if (io.kind == PTR_HOST) sync = true;
        return MODEM_OK;
    }
    modem_status finish() {
        if (sync) HIP_TRY(hipStreamSynchronize(s));
        return MODEM_OK;
    }
};

// capi_phasor.cpp
modem_status phasor_bps(const modem_phasor_desc* d, uint32_t* bps);
inline bool phasor_scanned(int kind) {          // phase carried from symbol to symbol (tx_scan)
    return kind == MODEM_PHASOR_DMPSK || kind == MODEM_PHASOR_MFSK || kind == MODEM_PHASOR_BFSK;
}
inline bool phasor_sample_dependent(int kind) {
    return kind == MODEM_PHASOR_DCQPSK || kind == MODEM_PHASOR_CPFSK || kind == MODEM_PHASOR_MSK ||
           phasor_scanned(kind);
}
// capi_chan.cpp: frac(v / (2 pi)) * 2^64 (the NCO words of the channel and the carrier synchronizer)
uint64_t chan_turns(double v);

}  // namespace capi
