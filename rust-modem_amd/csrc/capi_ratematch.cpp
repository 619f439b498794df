// rust-modem_amd/csrc/capi_ratematch.cpp — C ABI, host side: rate matching (puncturing, block interleaver) and the CRC.
#include "capi_common.h"
#include "modem_ratematch_math.h"

using namespace capi;

// The pattern, the interleaver and the frame of a call, checked and worked out; false: INVALID_ARG.
static bool rm_setup(const uint8_t* pattern, uint32_t P, uint32_t cols, size_t nm, mk::RmParams& p) {
    if (!pattern || P < 1 || P > (uint32_t)mk::kRmMaxP || cols < 1 || cols > (uint32_t)mk::kRmMaxCols || nm < 1 ||
        nm > (size_t)mk::kRmMaxNm)
        return false;
    uint64_t mask = 0;
    for (uint32_t i = 0; i < P; ++i) {
        if (pattern[i] > 1) return false;
        mask |= (uint64_t)pattern[i] << i;
    }
    p.mask = mask;
    p.P = P;
    p.w = mk::rm_popcount(mask);
    p.nm = (uint32_t)nm;
    p.E = mk::rm_kept(mask, P, p.nm);
    if (p.w < 1 || p.E < 1) return false;
    p.C = cols;
    p.rows = mk::rm_rows(p.E, cols);
    p.cl = p.E - (p.rows - 1) * cols;
    return true;
}

// The bytes [a, a + na) and [b, b + nb) share one.
static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
}

// Bytes from the first of nframes rows to the end of the last: rows of `row` elements, `stride` apart.
static size_t span_bytes(size_t nframes, size_t stride, size_t row, size_t esz) { return ((nframes - 1) * stride + row) * esz; }

static bool rows_fit(size_t nframes, size_t stride, size_t esz) { return !nframes || nframes <= SIZE_MAX / esz / stride; }

static bool crc_ok(uint32_t W, uint32_t poly, uint32_t init, uint32_t xorout, size_t nbits) {
    if (W != 8 && W != 16 && W != 24 && W != 32) return false;
    if ((poly | init | xorout) & ~mk::crc_mask(W)) return false;
    return nbits >= 1 && nbits <= (size_t)mk::kCrcMaxBits;
}

extern "C" {

modem_status modem_rm_kept(const uint8_t* pattern, uint32_t P, size_t nm, size_t* kept) {
    mk::RmParams p{};
    if (!kept || !rm_setup(pattern, P, 1, nm, p)) return MODEM_ERR_INVALID_ARG;
    *kept = p.E;
    return MODEM_OK;
}

modem_status modem_rm_tx(const uint8_t* pattern, uint32_t P, uint32_t cols, const uint8_t* bits, size_t nframes, size_t nm,
                         size_t in_stride, uint8_t* out, size_t out_stride, int device, void* stream) {
    mk::RmParams p{};
    if (!rm_setup(pattern, P, cols, nm, p) || in_stride < nm || out_stride < p.E || (nframes && (!bits || !out)))
        return MODEM_ERR_INVALID_ARG;
    if (!rows_fit(nframes, in_stride, 1) || !rows_fit(nframes, out_stride, 1)) return MODEM_ERR_INVALID_ARG;
    if (nframes && ranges_overlap(bits, span_bytes(nframes, in_stride, nm, 1), out, span_bytes(nframes, out_stride, p.E, 1)))
        return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    if (nframes == 0) return MODEM_OK;
    const HostIo io{device, (hipStream_t)stream};                   // device memory only: nothing is staged
    IoPtr b(bits), y(out);
    if (!io.take(b, 1, true) || !io.take(y, 1, true)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    p.in = bits;
    p.out = out;
    p.nframes = nframes;
    p.in_stride = in_stride;
    p.out_stride = out_stride;
    HIP_TRY(mk::launch_rm_tx(p, io.s));
    return MODEM_OK;
}

modem_status modem_rm_rx(const uint8_t* pattern, uint32_t P, uint32_t cols, int32_t dtype, const void* llr, size_t nframes,
                         size_t nm, size_t in_stride, const uint8_t* ok, void* out, size_t out_stride, int device, void* stream) {
    mk::RmParams p{};
    if (!rm_setup(pattern, P, cols, nm, p) || !llr_dtype_ok(dtype) || in_stride < p.E || out_stride < nm ||
        (nframes && (!llr || !out)))
        return MODEM_ERR_INVALID_ARG;
    const size_t esz = dtype_bytes(dtype);
    if (!rows_fit(nframes, in_stride, esz) || !rows_fit(nframes, out_stride, esz)) return MODEM_ERR_INVALID_ARG;
    if (nframes && ranges_overlap(llr, span_bytes(nframes, in_stride, p.E, esz), out, span_bytes(nframes, out_stride, nm, esz)))
        return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    if (nframes == 0) return MODEM_OK;
    const HostIo io{device, (hipStream_t)stream};
    IoPtr x(llr), y(out), k(ok);                                    // ok: accepted, checked as a pointer, not read
    if (!io.take(x, esz, true) || !io.take(y, esz, true) || !io.take(k, 1, true)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    p.in = llr;
    p.out = out;
    p.nframes = nframes;
    p.in_stride = in_stride;
    p.out_stride = out_stride;
    HIP_TRY(mk::launch_rm_rx(p, (int)esz, io.s));
    return MODEM_OK;
}

modem_status modem_crc_attach(uint32_t W, uint32_t poly, uint32_t init, uint32_t xorout, const uint8_t* bits, size_t nframes,
                              size_t nbits, size_t in_stride, uint8_t* out, size_t out_stride, int device, void* stream) {
    if (!crc_ok(W, poly, init, xorout, nbits) || in_stride < nbits || out_stride < nbits + W || (nframes && (!bits || !out)))
        return MODEM_ERR_INVALID_ARG;
    if (!rows_fit(nframes, in_stride, 1) || !rows_fit(nframes, out_stride, 1)) return MODEM_ERR_INVALID_ARG;
    if (nframes && ranges_overlap(bits, span_bytes(nframes, in_stride, nbits, 1), out, span_bytes(nframes, out_stride, nbits + W, 1)))
        return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    if (nframes == 0) return MODEM_OK;
    const HostIo io{device, (hipStream_t)stream};
    IoPtr b(bits), y(out);
    if (!io.take(b, 1, true) || !io.take(y, 1, true)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    mk::CrcParams p{};
    p.in = bits;
    p.out = out;
    p.nframes = nframes;
    p.in_stride = in_stride;
    p.out_stride = out_stride;
    p.nbits = (uint32_t)nbits;
    p.W = W;
    p.poly = poly;
    p.init = init;
    p.xorout = xorout;
    HIP_TRY(mk::launch_crc_attach(p, io.s));
    return MODEM_OK;
}

modem_status modem_crc_check(uint32_t W, uint32_t poly, uint32_t init, uint32_t xorout, const uint8_t* bits, size_t nframes,
                             size_t nbits, size_t in_stride, const uint8_t* ok_in, uint8_t* ok_out, int device, void* stream) {
    if (!crc_ok(W, poly, init, xorout, nbits) || in_stride < nbits + W || (nframes && (!bits || !ok_out)))
        return MODEM_ERR_INVALID_ARG;
    if (!rows_fit(nframes, in_stride, 1)) return MODEM_ERR_INVALID_ARG;
    if (nframes && ranges_overlap(bits, span_bytes(nframes, in_stride, nbits + W, 1), ok_out, nframes)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    if (nframes == 0) return MODEM_OK;
    const HostIo io{device, (hipStream_t)stream};
    IoPtr b(bits), ki(ok_in), ko(ok_out);
    if (!io.take(b, 1, true) || !io.take(ki, 1, true) || !io.take(ko, 1, true)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    mk::CrcParams p{};
    p.in = bits;
    p.out = ok_out;
    p.ok_in = ok_in;
    p.nframes = nframes;
    p.in_stride = in_stride;
    p.nbits = (uint32_t)nbits;
    p.W = W;
    p.poly = poly;
    p.init = init;
    p.xorout = xorout;
    HIP_TRY(mk::launch_crc_check(p, io.s));
    return MODEM_OK;
}

}  // extern "C"
