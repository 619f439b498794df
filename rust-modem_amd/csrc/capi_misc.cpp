// rust-modem_amd/csrc/capi_misc.cpp — C ABI, host side: the ABI version, bit-error counting and the device PRNG.
#include "capi_common.h"

using namespace capi;

extern "C" {

int32_t modem_abi_version(void) { return MODEM_HIP_ABI_VERSION; }

modem_status modem_count_errors(const uint8_t* a, const uint8_t* b, size_t n, uint64_t* counts, int device, void* stream) {
    if (!counts || (n && (!a || !b))) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    const PtrKind kc = ptr_kind(counts, device);
    if (kc == PTR_FOREIGN || (kc == PTR_DEVICE && reinterpret_cast<uintptr_t>(counts) % 8)) return MODEM_ERR_INVALID_ARG;
    if (n && (ptr_kind(a, device) != kc || ptr_kind(b, device) != kc)) return MODEM_ERR_INVALID_ARG;   // all device or all host
    if (n == 0) return MODEM_OK;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    hipStream_t s = (hipStream_t)stream;
    if (kc == PTR_DEVICE) {
        HIP_TRY(mk::launch_count_errors(a, b, n, counts, s));
        return MODEM_OK;
    }
    // host memory: staged through buffers of this call, synchronous
    Stage sa, sb, sc;
    modem_status st;
    if ((st = sa.ensure(n)) || (st = sb.ensure(n)) || (st = sc.ensure(2 * sizeof(uint64_t)))) return st;
    uint64_t got[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(sa.p, a, n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(sb.p, b, n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(sc.p, 0, sizeof(got), s));
    HIP_TRY(mk::launch_count_errors(static_cast<const uint8_t*>(sa.p), static_cast<const uint8_t*>(sb.p), n,
                                    static_cast<uint64_t*>(sc.p), s));
    HIP_TRY(hipMemcpyAsync(got, sc.p, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    counts[0] += got[0];
    counts[1] += got[1];
    return MODEM_OK;
}

modem_status modem_prng_bits(uint64_t seed, uint8_t* out, size_t nbits, int device, void* stream) {
    if (nbits && !out) return MODEM_ERR_INVALID_ARG;
    if (nbits && ptr_kind(out, device) != PTR_DEVICE) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    HIP_TRY(mk::launch_prng_bits(seed, out, nbits, (hipStream_t)stream));
    return MODEM_OK;
}

}  // extern "C"
