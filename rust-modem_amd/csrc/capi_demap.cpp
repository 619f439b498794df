// rust-modem_amd/csrc/capi_demap.cpp — C ABI, host side: the soft demapper.
#include "capi_common.h"
#include <cmath>
#include <cstring>

using namespace capi;

struct modem_demap {
    int device = 0;
    uint32_t bps = 0;
    int32_t in_dtype = 0, out_dtype = 0;
    bool axis = false;
    float* d_tab = nullptr;   // general: the 2^bps (i, q) points; axis: the I levels, then the Q levels
    Stage in_stage, out_stage;
    ~modem_demap() {
        DeviceGuard g(device);
        if (d_tab) (void)hipFree(d_tab);
    }
};

// The table is a product grid with an even bit split, bitwise: lut[2((a<<h)|b)] depends only on
// a, lut[2((a<<h)|b)+1] only on b (h = bps/2). levels: its 2^h I values, then its 2^h Q values —
// the table's own floats, so the axis path's inputs are the general path's.
static bool demap_axis_levels(const float* lut, uint32_t bps, std::vector<float>* levels) {
    if (bps % 2) return false;
    const uint32_t h = bps / 2, n = 1u << h;
    levels->resize(2 * n);
    for (uint32_t a = 0; a < n; ++a) {
        (*levels)[a] = lut[2 * (a << h)];
        (*levels)[n + a] = lut[2 * a + 1];
    }
    for (uint32_t a = 0; a < n; ++a)
        for (uint32_t b = 0; b < n; ++b) {
            const float* pt = lut + 2 * ((a << h) | b);
            if (std::memcmp(&pt[0], &(*levels)[a], sizeof(float)) != 0 ||
                std::memcmp(&pt[1], &(*levels)[n + b], sizeof(float)) != 0) return false;
        }
    return true;
}

extern "C" {

modem_status modem_demap_create(const float* lut, uint32_t bits_per_symbol, int32_t in_dtype, int32_t out_dtype,
                                int32_t path, int device, modem_demap** out) {
    if (!out) return MODEM_ERR_INVALID_ARG;
    *out = nullptr;
    if (!lut || bits_per_symbol < 1 || bits_per_symbol > 8) return MODEM_ERR_INVALID_ARG;
    if (!iq_dtype_ok(in_dtype) || !llr_dtype_ok(out_dtype)) return MODEM_ERR_INVALID_ARG;
    if (path != MODEM_DEMAP_AUTO && path != MODEM_DEMAP_GENERAL) return MODEM_ERR_INVALID_ARG;
    NEW_HANDLE(modem_demap, h, device);
    h->bps = bits_per_symbol;
    h->in_dtype = in_dtype;
    h->out_dtype = out_dtype;
    std::vector<float> levels;
    h->axis = path == MODEM_DEMAP_AUTO && demap_axis_levels(lut, bits_per_symbol, &levels);
    const float* tab = h->axis ? levels.data() : lut;
    const size_t ntab = h->axis ? levels.size() : (size_t)2 << bits_per_symbol;
    modem_status st;
    if ((st = upload(&h->d_tab, tab, ntab))) return st;
    *out = h.release();
    return MODEM_OK;
}

modem_status modem_demap_process(modem_demap* h, const void* iq, size_t nsym, float scale, void* llr, size_t cap,
                                 void* stream) {
    if (!h || !std::isfinite(scale) || (nsym && (!iq || !llr))) return MODEM_ERR_INVALID_ARG;
    if (nsym > SIZE_MAX / 8) return MODEM_ERR_INVALID_ARG;
    const size_t nllr = nsym * h->bps;
    if (cap < nllr) return MODEM_ERR_CAPACITY;
    if (nsym == 0) return MODEM_OK;
    const size_t isz = dtype_bytes(h->in_dtype), ob = dtype_bytes(h->out_dtype);
    HostIo io{h->device, (hipStream_t)stream};
    IoPtr x(iq), y(llr);
    // device pointers must be element-aligned (the kernel picks its access widths from there up)
    if (!io.take(x, isz) || !io.take(y, ob)) return MODEM_ERR_INVALID_ARG;
    DeviceGuard g(h->device);
    if (!g.ok) return MODEM_ERR_NO_DEVICE;
    modem_status st;
    if ((st = io.in(x, h->in_stage, nsym * 2 * isz)) || (st = io.out(y, h->out_stage, nllr * ob))) return st;
    mk::DemapParams p{};
    p.iq = x.dev;
    p.llr = y.dev;
    p.tab = h->d_tab;
    p.nsym = (int64_t)nsym;
    p.scale = scale;
    p.bps = (int32_t)h->bps;
    HIP_TRY(mk::launch_demap(p, h->axis, h->in_dtype, h->out_dtype, io.s));
    if ((st = io.back(y, nllr * ob))) return st;
    return io.finish();
}

int modem_demap_path(const modem_demap* h) { return h ? (h->axis ? 1 : 0) : -1; }

modem_status modem_demap_destroy(modem_demap* h) { delete h; return MODEM_OK; }

}  // extern "C"
