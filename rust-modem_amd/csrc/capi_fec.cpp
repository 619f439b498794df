// rust-modem_amd/csrc/capi_fec.cpp — C ABI, host side: the convolutional encoder and the batched Viterbi decoder.
#include "capi_common.h"
#include "modem_fec_math.h"
#include <cmath>

using namespace capi;

static bool conv_code_ok(uint32_t K, const uint32_t* polys, uint32_t n, uint32_t flags) {
    if (K < (uint32_t)mk::kFecMinK || K > (uint32_t)mk::kFecMaxK || (n != 2 && n != 3) || !polys) return false;
    if (flags & ~(uint32_t)MODEM_CONV_TAIL) return false;
    for (uint32_t j = 0; j < n; ++j)
        if (polys[j] == 0 || polys[j] >= (1u << K)) return false;
    return true;
}

// Host side: the code; device side: its S branch words, nothing that a call changes.
struct modem_viterbi {
    int device = 0;
    int32_t K = 0, n = 0, tail = 0, in_dtype = 0;
    uint32_t* d_table = nullptr;
    ~modem_viterbi() {
        DeviceGuard g(device);
        if (d_table) (void)hipFree(d_table);
    }
};

extern "C" {

modem_status modem_conv_encode(uint32_t K, const uint32_t* polys, uint32_t n, uint32_t flags, const uint8_t* bits,
                               size_t nframes, size_t nbits, size_t in_stride, uint8_t* out, size_t out_stride, int device,
                               void* stream) {
    if (!conv_code_ok(K, polys, n, flags) || nbits == 0 || nbits > SIZE_MAX / 8 || in_stride < nbits) return MODEM_ERR_INVALID_ARG;
    const size_t T = nbits + ((flags & MODEM_CONV_TAIL) ? K - 1 : 0);
    if (out_stride / n < T || (nframes && (!bits || !out))) return MODEM_ERR_INVALID_ARG;
    if (nframes && (nframes > SIZE_MAX / in_stride || nframes > SIZE_MAX / out_stride)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(device)) return MODEM_ERR_NO_DEVICE;
    if (nframes == 0) return MODEM_OK;
    const HostIo io{device, (hipStream_t)stream};                   // device memory only: nothing is staged
    IoPtr b(bits), y(out);
    if (!io.take(b, 1, true) || !io.take(y, 1, true)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    mk::ConvEncodeParams p{};
    p.bits = bits;
    p.out = out;
    p.nframes = nframes;
    p.nbits = nbits;
    p.T = T;
    p.in_stride = in_stride;
    p.out_stride = out_stride;
    for (uint32_t j = 0; j < n; ++j) p.g[j] = polys[j];
    p.K = (int32_t)K;
    p.n = (int32_t)n;
    HIP_TRY(mk::launch_conv_encode(p, io.s));
    return MODEM_OK;
}

modem_status modem_viterbi_create(uint32_t K, const uint32_t* polys, uint32_t n, uint32_t flags, int32_t in_dtype, int device,
                                  modem_viterbi** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!conv_code_ok(K, polys, n, flags) || !llr_dtype_ok(in_dtype)) return MODEM_ERR_INVALID_ARG;
    NEW_HANDLE(modem_viterbi, h, device);
    h->K = (int32_t)K;
    h->n = (int32_t)n;
    h->tail = (flags & MODEM_CONV_TAIL) ? 1 : 0;
    h->in_dtype = in_dtype;
    const uint32_t S = 1u << (K - 1);
    std::vector<uint32_t> table(S);
    for (uint32_t s = 0; s < S; ++s) table[s] = mk::fec_branch_word(s, (int)K, polys, (int)n);
    modem_status st;
    if ((st = upload(&h->d_table, table.data(), (size_t)S))) return st;
    *out = h.release();
    return MODEM_OK;
}

modem_status modem_viterbi_process(modem_viterbi* h, const void* llr, size_t stride, size_t nframes, size_t nbits, float qscale,
                                   const uint8_t* ok, uint8_t* out, size_t out_stride, int32_t* metric, void* stream) {
    if (!h || nbits == 0 || !std::isfinite(qscale) || !(qscale > 0.0f)) return MODEM_ERR_INVALID_ARG;
    const size_t maxT = (size_t)mk::fec_max_steps(h->K), tailn = h->tail ? (size_t)(h->K - 1) : 0;
    if (nbits > maxT || nbits + tailn > maxT) return MODEM_ERR_INVALID_ARG;
    const size_t T = nbits + tailn, esz = dtype_bytes(h->in_dtype);
    if (stride < (size_t)h->n * T || out_stride < nbits || (nframes && (!llr || !out))) return MODEM_ERR_INVALID_ARG;
    if (nframes && (nframes > SIZE_MAX / esz / stride || nframes > SIZE_MAX / out_stride)) return MODEM_ERR_INVALID_ARG;
    if (!device_ok(h->device)) return MODEM_ERR_NO_DEVICE;
    if (nframes == 0) return MODEM_OK;
    const HostIo io{h->device, (hipStream_t)stream};                // device memory only: nothing is staged
    IoPtr x(llr), y(out), k(ok), mt(metric);
    if (!io.take(x, esz, true) || !io.take(y, 1, true) || !io.take(k, 1, true) || !io.take(mt, 4, true))
        return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    mk::ViterbiParams p{};
    p.llr = llr;
    p.ok = ok;
    p.table = h->d_table;
    p.out = out;
    p.metric = metric;
    p.nframes = nframes;
    p.stride = stride;
    p.out_stride = out_stride;
    p.qscale = qscale;
    p.K = h->K;
    p.n = h->n;
    p.tail = h->tail;
    p.nbits = (int32_t)nbits;
    p.T = (int32_t)T;
    HIP_TRY(mk::launch_viterbi(p, h->in_dtype, (hipStream_t)stream));
    return MODEM_OK;
}

modem_status modem_viterbi_destroy(modem_viterbi* h) { delete h; return MODEM_OK; }

}  // extern "C"
