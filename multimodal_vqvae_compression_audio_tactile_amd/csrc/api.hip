// api.hip -- the C ABI of libmvq_hip.so (declared in include/mvq.h): argument checks and kernel dispatch.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include "../../include/mvq.h"
#include "conv_dispatch.hpp"
#include "kernels_small.hpp"

#include <map>
#include <string>
#include <vector>

namespace mvq {
// ---- per-launch HIP-event profiler ------------------------------------------------------------------------------------
namespace {
struct ProfRec { std::string name; double flops; hipEvent_t e0, e1; };
std::vector<ProfRec> g_prof;
std::vector<hipEvent_t> g_prof_pool;          // events are reused between sessions
bool g_prof_on = false;
hipError_t g_prof_err = hipSuccess;           // first hipEventCreate / hipEventRecord failure of the session (reported by _end)
hipEvent_t prof_event()
{
    if (!g_prof_pool.empty()) { hipEvent_t e = g_prof_pool.back(); g_prof_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    const hipError_t rc = hipEventCreate(&e);
    if (rc != hipSuccess) { if (g_prof_err == hipSuccess) g_prof_err = rc; return nullptr; }
    return e;
}
}  // namespace
bool prof_enabled() { return g_prof_on; }
int prof_begin(const char* kernel_name, double flops, hipStream_t s)
{
    if (!g_prof_on) return -1;
    ProfRec r{kernel_name, flops, prof_event(), nullptr};
    if (!r.e0) return -1;
    r.e1 = prof_event();
    if (!r.e1) { g_prof_pool.push_back(r.e0); return -1; }      // do not leak the first event when the second cannot be made
    const hipError_t rc = hipEventRecord(r.e0, s);
    if (rc != hipSuccess) {
        if (g_prof_err == hipSuccess) g_prof_err = rc;
        g_prof_pool.push_back(r.e0); g_prof_pool.push_back(r.e1);
        return -1;
    }
    g_prof.push_back(r);
    return (int)g_prof.size() - 1;
}
void prof_end(int idx, hipStream_t s)
{
    if (idx < 0 || idx >= (int)g_prof.size()) return;
    const hipError_t rc = hipEventRecord(g_prof[idx].e1, s);
    if (rc != hipSuccess && g_prof_err == hipSuccess) g_prof_err = rc;
}
}  // namespace mvq

namespace {
thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return code;
}
int hipfail(hipError_t e, const char* what)
{
    return fail(MVQ_EHIP, "%s: %s", what, hipGetErrorString(e));
}
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
}  // namespace
namespace mvq {
// stacks.hip reports through the same mvq_last_error() text
void set_last_error(const char* msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }
}
namespace {
inline int conv_out_len(int tin, int ks, int stride, int dil, int pad)
{
    const int span = tin + 2 * pad - dil * (ks - 1) - 1;
    return span < 0 ? 0 : span / stride + 1;
}
}  // namespace

extern "C" {

int mvq_profile_begin(void)
{
    for (auto& r : mvq::g_prof) { mvq::g_prof_pool.push_back(r.e0); mvq::g_prof_pool.push_back(r.e1); }
    mvq::g_prof.clear();
    mvq::g_prof_err = hipSuccess;
    mvq::g_prof_on = true;
    return MVQ_OK;
}

int mvq_profile_reserve(int n_launches)
{
    /* create the event pairs of `n_launches` launches ahead of time, so that no hipEventCreate falls into a timed region */
    if (n_launches < 0) return fail(MVQ_EINVAL, "profile_reserve: negative count");
    std::vector<hipEvent_t> made;
    const size_t want = 2 * (size_t)n_launches;
    while (mvq::g_prof_pool.size() + made.size() < want) {
        hipEvent_t e = nullptr;
        const hipError_t rc = hipEventCreate(&e);
        if (rc != hipSuccess) { for (auto m : made) mvq::g_prof_pool.push_back(m); return hipfail(rc, "profile_reserve: hipEventCreate"); }
        made.push_back(e);
    }
    for (auto m : made) mvq::g_prof_pool.push_back(m);
    return MVQ_OK;
}

int mvq_profile_end(mvq_profile_entry* out, int max_entries, int* n_entries)
{
    return mvq_profile_end2(out, max_entries, n_entries, nullptr);
}

int mvq_profile_end2(mvq_profile_entry* out, int max_entries, int* n_entries, int* n_total)
{
    /* *n_entries = rows WRITTEN (<= max_entries); kernels beyond max_entries are dropped, never written past the buffer;
     * *n_total = instantiations the session saw (> *n_entries means the buffer truncated the table) */
    mvq::g_prof_on = false;
    if (n_total) *n_total = 0;
    if (!n_entries || max_entries < 0 || (max_entries > 0 && !out)) return fail(MVQ_EINVAL, "profile_end: bad argument");
    *n_entries = 0;
    auto recycle = [] {
        for (auto& r : mvq::g_prof) { mvq::g_prof_pool.push_back(r.e0); mvq::g_prof_pool.push_back(r.e1); }
        mvq::g_prof.clear();
    };
    if (mvq::g_prof_err != hipSuccess) {
        const hipError_t e = mvq::g_prof_err;
        mvq::g_prof_err = hipSuccess;
        recycle();
        return hipfail(e, "profile: an event could not be created or recorded during the session");
    }
    std::map<std::string, mvq_profile_entry> agg;
    for (auto& r : mvq::g_prof) {
        hipError_t e = hipEventSynchronize(r.e1);
        if (e != hipSuccess) { recycle(); return hipfail(e, "profile_end: hipEventSynchronize"); }
        float ms = 0.0f;
        e = hipEventElapsedTime(&ms, r.e0, r.e1);
        if (e != hipSuccess) { recycle(); return hipfail(e, "profile_end: hipEventElapsedTime"); }
        auto it = agg.find(r.name);
        if (it == agg.end()) {
            mvq_profile_entry z{};
            snprintf(z.kernel, sizeof(z.kernel), "%s", r.name.c_str());
            it = agg.emplace(r.name, z).first;
        }
        it->second.seconds += 1e-3 * (double)ms;
        it->second.flops += r.flops;
        it->second.launches += 1;
    }
    recycle();
    int i = 0;
    for (auto& kv : agg) {
        if (i >= max_entries) break;
        out[i++] = kv.second;
    }
    *n_entries = i;
    if (n_total) *n_total = (int)agg.size();
    return MVQ_OK;
}

int mvq_abi_version(void) { return 3; }
unsigned mvq_build_flags(void) { return getenv("MVQ_NO_DMA") ? 0x100u : 0u; }
const char* mvq_last_error(void) { return g_err; }

int mvq_device_query(int* cu_count, int* lds_bytes_per_cu, char* arch, int arch_len)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return hipfail(e, "hipGetDevice");
    hipDeviceProp_t p;
    e = hipGetDeviceProperties(&p, dev);
    if (e != hipSuccess) return hipfail(e, "hipGetDeviceProperties");
    if (cu_count) *cu_count = p.multiProcessorCount;
    if (lds_bytes_per_cu) *lds_bytes_per_cu = (int)p.maxSharedMemoryPerMultiProcessor;
    if (arch && arch_len > 0) { strncpy(arch, p.gcnArchName, arch_len - 1); arch[arch_len - 1] = 0; }
    return MVQ_OK;
}

int mvq_weight_norm_f32(const float* v, const float* g, float* w, int rows, int inner, void* stream)
{
    if (!v || !g || !w || rows <= 0 || inner <= 0) return fail(MVQ_EINVAL, "weight_norm: bad argument");
    hipError_t e = mvq::launch_weight_norm(v, g, w, rows, inner, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "weight_norm");
}

size_t mvq_conv1d_packed_floats(int cin, int cout, int ks)
{
    if (cin <= 0 || cout <= 0 || ks <= 0) return 0;
    return (size_t)cin * ks * mvq::conv_mpad(cout);
}

int mvq_conv1d_pack_f32(const float* w, float* wp, int cin, int cout, int ks, void* stream)
{
    if (!w || !wp || cin <= 0 || cout <= 0 || ks <= 0) return fail(MVQ_EINVAL, "conv1d_pack: bad argument");
    hipError_t e = mvq::launch_pack_conv1d(w, wp, cin, cout, ks, mvq::conv_mpad(cout), S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_pack");
}

size_t mvq_conv_transpose1d_packed_floats(int cin, int cout, int stride)
{
    if (cin <= 0 || cout <= 0 || stride <= 0) return 0;
    return (size_t)cin * 2 * mvq::conv_mpad(cout * stride);
}

int mvq_conv_transpose1d_pack_f32(const float* w, float* wp, int cin, int cout, int stride, void* stream)
{
    if (!w || !wp || cin <= 0 || cout <= 0 || stride <= 0) return fail(MVQ_EINVAL, "conv_transpose1d_pack: bad argument");
    hipError_t e = mvq::launch_pack_convtr(w, wp, cin, cout, stride, mvq::conv_mpad(cout * stride), S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv_transpose1d_pack");
}

static hipError_t dispatch_conv1d(const mvq::ConvArgs& a, int ks, int stride, int dil, hipStream_t s)
{
    const int bm = mvq::conv_tile_bm(a.Cout);
    hipError_t e = hipErrorInvalidValue;
    /* latency regime (one segment, a batch of six: conv_lat.hip): the 128-row tiling would put a block on fewer than 160 of the
     * 256 CUs and the launch has few enough 16 x 16 tiles -> one wave per tile on v_mfma_f32_16x16x4_f32, same fma chains */
    if (a.Cout >= 16 && a.Cin >= 32 && mvq::conv_underfilled(a) && mvq::conv_lat_wanted(a, ks)) {
        e = mvq::launch_conv_lat(a, ks, stride, dil, s);
        if (e != hipErrorInvalidValue) return e;
    }
    if (a.Cout >= 32 && a.Cin >= 32) {                 // a dense (channels x kernel) tile exists
        if (ks == 7 && stride == 1 && a.Cin % 8 == 0) e = mvq::launch_conv_k7(a, dil, bm, s);
        else if (ks == 1 && stride == 1 && dil == 1 && a.Cin % 32 == 0) e = mvq::launch_conv_k1k3(a, 1, bm, s);
        else if (ks == 3 && stride == 1 && dil == 1 && a.Cin % 16 == 0) e = mvq::launch_conv_k1k3(a, 3, bm, s);
        else if (ks == 2 * stride && dil == 1 && a.Cin % 16 == 0) e = mvq::launch_conv_strided(a, stride, bm, s);
    }
    return e;
}

static hipError_t dispatch_convtr(const mvq::ConvArgs& a, hipStream_t s)
{
    if (a.Cin % 32 != 0 || a.Mrows < 64) return hipErrorInvalidValue;
    return mvq::launch_conv_tr(a, mvq::conv_tile_bm(a.Mrows), s);
}

/* ---- opt-in bf16x6 arithmetic mode (conv_k7_bf16.hip; include/mvq.h) ---- */
size_t mvq_bf16x3_split_bytes(int batch, int c, int t)
{
    if (batch <= 0 || c <= 0 || t <= 0) return 0;
    return (size_t)batch * c * t * 6;
}
int mvq_bf16x3_split_f32(const float* x, void* xs, int batch, int c, int t, void* stream)
{
    if (batch < 0 || c <= 0 || t < 0 || c % 8 != 0) return fail(MVQ_EINVAL, "bf16x3_split: bad shape B=%d C=%d T=%d (C %% 8 == 0)", batch, c, t);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!x || !xs) return fail(MVQ_EINVAL, "bf16x3_split: null tensor");
    if ((reinterpret_cast<uintptr_t>(xs) & 15) != 0) return fail(MVQ_EINVAL, "bf16x3_split: xs must be 16-byte aligned");
    const hipError_t e = mvq::launch_bf16x3_split(x, xs, batch, c, t, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "bf16x3_split");
}
size_t mvq_conv1d_k7_bf16x3_packed_bytes(int cout, int cin)
{
    if (cout <= 0 || cin <= 0 || mvq::bf16x6_tile_rows(cout) == 0 || cin % 16 != 0) return 0;
    return (size_t)cout * cin * 7 * 6;
}
int mvq_conv1d_k7_pack_bf16x3(const float* w, void* wq, int cout, int cin, int dgrad, void* stream)
{
    if (cout <= 0 || cin <= 0 || mvq::bf16x6_tile_rows(cout) == 0 || cin % 16 != 0)
        return fail(MVQ_EINVAL, "conv1d_k7_pack_bf16x3: Cout %d must be a multiple of 128 or 96 and Cin %d of 16", cout, cin);
    if (!w || !wq) return fail(MVQ_EINVAL, "conv1d_k7_pack_bf16x3: null tensor");
    if ((reinterpret_cast<uintptr_t>(wq) & 15) != 0) return fail(MVQ_EINVAL, "conv1d_k7_pack_bf16x3: wq must be 16-byte aligned");
    const hipError_t e = mvq::launch_bf16x3_pack_k7(w, wq, cout, cin, dgrad != 0, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_k7_pack_bf16x3");
}
int mvq_conv1d_k7_bf16x6_f32(const void* xs, const void* wq, const float* bias, const float* alpha_out, float* y, float* y2,
                             const float* dsn_src, const float* dsn_alpha, const float* residual,
                             int batch, int cin, int t, int cout, int dil, int tvalid, void* stream)
{
    if (batch < 0 || cin <= 0 || cout <= 0 || t < 0 || mvq::bf16x6_tile_rows(cout) == 0 || cin % 16 != 0)
        return fail(MVQ_EINVAL, "conv1d_k7_bf16x6: bad shape B=%d Cin=%d T=%d Cout=%d (Cout %% 128 or 96, Cin %% 16)", batch, cin, t, cout);
    if (dil != 1 && dil != 3 && dil != 9) return fail(MVQ_EINVAL, "conv1d_k7_bf16x6: dilation %d not in {1, 3, 9}", dil);
    if (tvalid < 0 || tvalid > t) return fail(MVQ_EINVAL, "conv1d_k7_bf16x6: tvalid %d outside [0, %d]", tvalid, t);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!xs || !wq || !y) return fail(MVQ_EINVAL, "conv1d_k7_bf16x6: null tensor");
    if (((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(wq)) & 15) != 0)
        return fail(MVQ_EINVAL, "conv1d_k7_bf16x6: xs / wq must be 16-byte aligned");
    if ((long long)batch * ((t + 127) / 128) > 0x7fffffffLL) return fail(MVQ_EINVAL, "conv1d_k7_bf16x6: grid too large");
    if (y2 && !alpha_out) return fail(MVQ_EINVAL, "conv1d_k7_bf16x6: the dual output needs alpha_out");
    if ((dsn_src != nullptr) != (dsn_alpha != nullptr)) return fail(MVQ_EINVAL, "conv1d_k7_bf16x6: dsn_src and dsn_alpha go together");
    mvq::K7Extra ex; ex.y2 = y2; ex.dsn_src = dsn_src; ex.dsn_alpha = dsn_alpha; ex.residual = residual;
    const hipError_t e = mvq::launch_conv_k7_bf16x6(xs, wq, bias, alpha_out, y, batch, cin, t, cout, dil, tvalid, ex, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_k7_bf16x6");
}

/* f16x3 form of the opt-in mode (include/mvq.h) */
int mvq_f16x2_split_f32(const float* x, void* xs, uint32_t* xamax, int batch, int c, int t, void* stream)
{
    if (batch < 0 || c <= 0 || t < 0 || c % 8 != 0) return fail(MVQ_EINVAL, "f16x2_split: bad shape B=%d C=%d T=%d (C %% 8 == 0)", batch, c, t);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!x || !xs || !xamax) return fail(MVQ_EINVAL, "f16x2_split: null tensor");
    if ((reinterpret_cast<uintptr_t>(xs) & 15) != 0) return fail(MVQ_EINVAL, "f16x2_split: xs must be 16-byte aligned");
    const hipError_t e = mvq::launch_f16x2_split(x, xs, xamax, batch, c, t, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "f16x2_split");
}
size_t mvq_conv1d_k7_f16x2_packed_bytes(int cout, int cin)
{
    if (cout <= 0 || cin <= 0 || mvq::bf16x6_tile_rows(cout) == 0 || cin % 16 != 0) return 0;
    return (size_t)cout * cin * 7 * 4;
}
int mvq_conv1d_k7_pack_f16x2(const float* w, void* wq, uint32_t* wamax, int cout, int cin, int dgrad, void* stream)
{
    if (cout <= 0 || cin <= 0 || mvq::bf16x6_tile_rows(cout) == 0 || cin % 16 != 0)
        return fail(MVQ_EINVAL, "conv1d_k7_pack_f16x2: Cout %d must be a multiple of 128 or 96 and Cin %d of 16", cout, cin);
    if (!w || !wq || !wamax) return fail(MVQ_EINVAL, "conv1d_k7_pack_f16x2: null tensor");
    if ((reinterpret_cast<uintptr_t>(wq) & 15) != 0) return fail(MVQ_EINVAL, "conv1d_k7_pack_f16x2: wq must be 16-byte aligned");
    const hipError_t e = mvq::launch_f16x2_pack_k7(w, wq, wamax, cout, cin, dgrad != 0, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_k7_pack_f16x2");
}
int mvq_conv1d_k7_f16x3_f32(const void* xs, const uint32_t* xamax, const void* wq, const uint32_t* wamax, const float* bias,
                            const float* alpha_out, float* y, float* y2, const float* dsn_src, const float* dsn_alpha,
                            const float* residual, int batch, int cin, int t, int cout, int dil, int tvalid, void* stream)
{
    if (batch < 0 || cin <= 0 || cout <= 0 || t < 0 || mvq::bf16x6_tile_rows(cout) == 0 || cin % 16 != 0)
        return fail(MVQ_EINVAL, "conv1d_k7_f16x3: bad shape B=%d Cin=%d T=%d Cout=%d (Cout %% 128 or 96, Cin %% 16)", batch, cin, t, cout);
    if (dil != 1 && dil != 3 && dil != 9) return fail(MVQ_EINVAL, "conv1d_k7_f16x3: dilation %d not in {1, 3, 9}", dil);
    if (tvalid < 0 || tvalid > t) return fail(MVQ_EINVAL, "conv1d_k7_f16x3: tvalid %d outside [0, %d]", tvalid, t);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!xs || !wq || !y || !xamax || !wamax) return fail(MVQ_EINVAL, "conv1d_k7_f16x3: null tensor");
    if (((reinterpret_cast<uintptr_t>(xs) | reinterpret_cast<uintptr_t>(wq)) & 15) != 0)
        return fail(MVQ_EINVAL, "conv1d_k7_f16x3: xs / wq must be 16-byte aligned");
    if ((long long)batch * ((t + 127) / 128) > 0x7fffffffLL) return fail(MVQ_EINVAL, "conv1d_k7_f16x3: grid too large");
    if (y2 && !alpha_out) return fail(MVQ_EINVAL, "conv1d_k7_f16x3: the dual output needs alpha_out");
    if ((dsn_src != nullptr) != (dsn_alpha != nullptr)) return fail(MVQ_EINVAL, "conv1d_k7_f16x3: dsn_src and dsn_alpha go together");
    mvq::K7Extra ex; ex.y2 = y2; ex.dsn_src = dsn_src; ex.dsn_alpha = dsn_alpha; ex.residual = residual;
    const hipError_t e = mvq::launch_conv_k7_f16x3(xs, xamax, wq, wamax, bias, alpha_out, y, batch, cin, t, cout, dil, tvalid, ex, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_k7_f16x3");
}

/* which kernel instantiation mvq_conv1d_f32 / mvq_conv_transpose1d_f32 launches for a shape (profiling aid):
 * runs the real dispatch in "name mode" */
int mvq_conv_kernel_name(int batch, int cin, int cout, int ks, int stride, int dil, int transposed, int tin, char* buf, int len)
{
    if (!buf || len <= 0) return fail(MVQ_EINVAL, "conv_kernel_name: bad buffer");
    mvq::ConvArgs a{};
    a.B = batch; a.Cin = cin; a.Tin = tin; a.Cout = cout; a.name_out = buf; a.name_len = len;
    hipError_t e;
    if (transposed) {
        a.Mrows = cout * stride; a.Mpad = mvq::conv_mpad(a.Mrows); a.Ncols = tin + 1; a.up_s = stride; a.pad = 1;
        e = dispatch_convtr(a, nullptr);
        if (e != hipSuccess) snprintf(buf, len, "convtr_direct_kernel");
    } else {
        const int pad = stride == 1 ? (ks - 1) * dil / 2 : (stride + 1) / 2;
        a.Mrows = cout; a.Mpad = mvq::conv_mpad(cout); a.Ncols = conv_out_len(tin, ks, stride, dil, pad); a.pad = pad;
        a.Tout = a.Ncols; a.up_s = 1;
        e = dispatch_conv1d(a, ks, stride, dil, nullptr);
        if (e != hipSuccess)
            snprintf(buf, len, "%s", (cin == 1 && ks == 7 && stride == 1 && dil == 1) ? "conv1d_cin1_kernel<7>"
                                   : (cout == 1 && ks == 7 && stride == 1 && dil == 1) ? "conv1d_cout1_kernel<7>"
                                                                                       : "conv1d_direct_kernel");
    }
    return MVQ_OK;
}

/* ... and which kernel the three forward launchers that choose by token count, width and alignment run (the launchers' own
 * decision functions: kernels_small.hpp).  Host arithmetic only: nothing is launched, no device is needed. */
int mvq_layernorm_kernel_name(int batch, int c, int t, char* buf, int len)
{
    if (!buf || len <= 0) return fail(MVQ_EINVAL, "layernorm_kernel_name: bad buffer");
    if (c <= 0 || batch <= 0 || t <= 0) return fail(MVQ_EINVAL, "layernorm_kernel_name: bad shape B=%d C=%d T=%d", batch, c, t);
    snprintf(buf, len, "%s", mvq::layernorm_form_name(mvq::layernorm_form(batch * t, c)));
    return MVQ_OK;
}
int mvq_rvq_ema_forward_kernel_name(int batch, int dim, int t, int k, int books_aligned, char* buf, int len)
{
    if (!buf || len <= 0) return fail(MVQ_EINVAL, "rvq_ema_forward_kernel_name: bad buffer");
    if (batch <= 0 || t <= 0 || dim <= 0 || dim > 128 || dim % 4 != 0 || k <= 0)
        return fail(MVQ_EINVAL, "rvq_ema_forward_kernel_name: bad shape B=%d D=%d T=%d K=%d", batch, dim, t, k);
    mvq::rvq_ema_forward_form_name(mvq::rvq_ema_forward_form(batch * t, dim, k, books_aligned != 0), buf, len);
    return MVQ_OK;
}
int mvq_dac_rvq_kernel_name(int batch, int c, int t, int k, int prepared, int aligned, char* buf, int len)
{
    if (!buf || len <= 0) return fail(MVQ_EINVAL, "dac_rvq_kernel_name: bad buffer");
    if (batch <= 0 || t <= 0 || k <= 0 || (c != 1024 && c != 512 && c != 256))
        return fail(MVQ_EINVAL, "dac_rvq_kernel_name: bad shape B=%d C=%d T=%d K=%d (C in {256,512,1024})", batch, c, t, k);
    mvq::dac_rvq_form_name(mvq::dac_rvq_form(batch * t, c, k, prepared != 0, aligned != 0), c, buf, len);
    return MVQ_OK;
}

int mvq_conv1d_dual_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                        const float* residual, const float* alpha_out, float* y, float* y2, const float* alpha2,
                        int batch, int cin, int tin, int cout, int ks, int stride, int dil, int pad, int act, void* stream);

int mvq_conv1d_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                   const float* residual, const float* alpha_out, float* y,
                   int batch, int cin, int tin, int cout, int ks, int stride, int dil, int pad, int act, void* stream)
{
    return mvq_conv1d_dual_f32(x, wp, bias, alpha_in, residual, alpha_out, y, nullptr, nullptr,
                               batch, cin, tin, cout, ks, stride, dil, pad, act, stream);
}

int mvq_conv1d_dual_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                        const float* residual, const float* alpha_out, float* y, float* y2, const float* alpha2,
                        int batch, int cin, int tin, int cout, int ks, int stride, int dil, int pad, int act, void* stream)
{
    return mvq_conv1d_padded_f32(x, wp, bias, alpha_in, residual, alpha_out, y, y2, alpha2, batch, cin, tin, cout, ks, stride,
                                 dil, pad, act, 0, stream);
}

int mvq_conv1d_padded_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                          const float* residual, const float* alpha_out, float* y, float* y2, const float* alpha2,
                          int batch, int cin, int tin, int cout, int ks, int stride, int dil, int pad, int act, int tvalid,
                          void* stream)
{
    if (batch < 0 || cin <= 0 || cout <= 0 || tin < 0 || ks <= 0 || stride <= 0 || dil <= 0 || pad < 0)
        return fail(MVQ_EINVAL, "conv1d: bad shape B=%d Cin=%d Tin=%d Cout=%d ks=%d s=%d d=%d p=%d", batch, cin, tin, cout, ks, stride, dil, pad);
    if (act != MVQ_ACT_NONE && act != MVQ_ACT_TANH && act != MVQ_ACT_GELU) return fail(MVQ_EINVAL, "conv1d: bad act %d", act);
    const int tout = conv_out_len(tin, ks, stride, dil, pad);
    if (batch == 0 || tout == 0) return MVQ_OK;
    if (!x || !wp || !y) return fail(MVQ_EINVAL, "conv1d: null tensor");
    if ((y2 != nullptr) != (alpha2 != nullptr)) return fail(MVQ_EINVAL, "conv1d: y2 and alpha2 go together");
    if (tvalid < 0 || tvalid > tout) return fail(MVQ_EINVAL, "conv1d: tvalid %d outside [0, %d]", tvalid, tout);
    const int mpad = mvq::conv_mpad(cout);

    mvq::ConvArgs a{};
    a.x = x; a.wp = wp; a.bias = bias; a.alpha_in = alpha_in; a.residual = residual; a.alpha_out = alpha_out; a.y = y;
    a.B = batch; a.Cin = cin; a.Tin = tin; a.Cout = cout; a.Tout = tout; a.pad = pad; a.Mpad = mpad;
    a.Mrows = cout; a.Ncols = tout; a.act = act; a.up_s = 1; a.up_p = 0; a.y2 = y2; a.alpha2 = alpha2;
    a.tvalid = (tvalid == tout) ? 0 : tvalid;

    hipError_t e = dispatch_conv1d(a, ks, stride, dil, S(stream));
    if (e == hipErrorInvalidValue && (a.tvalid || act == MVQ_ACT_GELU))
        return fail(MVQ_EUNSUPPORTED, "conv1d: zero-padded rows / the GELU epilogue need an MFMA-tiled shape");
    if (e == hipErrorInvalidValue) {
        (void)hipGetLastError();
        mvq::DirectConvArgs d{x, wp, bias, alpha_in, residual, alpha_out, y, batch, cin, tin, cout, tout, ks, stride, dil, pad, mpad, act, y2, alpha2, nullptr, nullptr};
        e = mvq::launch_conv1d_direct(d, S(stream));
    }
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d");
}

static unsigned magic_div(int d) { return (unsigned)((((unsigned long long)1 << 32) + (unsigned)d - 1) / (unsigned)d); }   /* umulhi(n, magic) == n / d for n * d < 2^32 */

int mvq_conv1d_packed_rows_f32(const float* x, const float* wp, const float* bias, const float* residual, const float* alpha_out,
                               float* y, float* y2, const float* alpha2, int rows, int cin, int cout, int ks, int dil, int pad,
                               int act, int seg_per_row, int seg_period, int seg_valid, void* stream)
{
    if (rows < 0 || cin <= 0 || cout <= 0 || ks <= 0 || dil <= 0 || pad < 0 || seg_per_row <= 0 || seg_period <= 0 || seg_valid < 0)
        return fail(MVQ_EINVAL, "conv1d_packed_rows: bad shape");
    if (seg_period % 4 != 0 || seg_valid > seg_period || (ks - 1) * dil != 2 * pad || pad > seg_period - seg_valid)
        return fail(MVQ_EINVAL, "conv1d_packed_rows: needs a 'same' stride-1 conv, a period that is a multiple of 4 and a gap of at "
                                "least `pad` zero columns between segments (period %d, valid %d, pad %d)", seg_period, seg_valid, pad);
    if (act != MVQ_ACT_NONE && act != MVQ_ACT_TANH && act != MVQ_ACT_GELU) return fail(MVQ_EINVAL, "conv1d_packed_rows: bad act %d", act);
    const long long t = (long long)seg_per_row * seg_period;
    if (t * seg_period >= ((long long)1 << 32)) return fail(MVQ_EINVAL, "conv1d_packed_rows: row too long");
    if (rows == 0 || seg_valid == 0) return MVQ_OK;
    if (!x || !wp || !y) return fail(MVQ_EINVAL, "conv1d_packed_rows: null tensor");
    if ((y2 != nullptr) != (alpha2 != nullptr)) return fail(MVQ_EINVAL, "conv1d_packed_rows: y2 and alpha2 go together");
    mvq::ConvArgs a{};
    a.x = x; a.wp = wp; a.bias = bias; a.residual = residual; a.alpha_out = alpha_out; a.y = y; a.y2 = y2; a.alpha2 = alpha2;
    a.B = rows; a.Cin = cin; a.Tin = (int)t; a.Cout = cout; a.Tout = (int)t; a.pad = pad; a.Mpad = mvq::conv_mpad(cout);
    a.Mrows = cout; a.Ncols = (int)t; a.act = act; a.up_s = 1;
    a.tper = seg_period; a.tper_valid = seg_valid; a.tper_magic = magic_div(seg_period);
    hipError_t e = dispatch_conv1d(a, ks, 1, dil, S(stream));
    if (e == hipErrorInvalidValue) return fail(MVQ_EUNSUPPORTED, "conv1d_packed_rows: needs an MFMA-tiled shape");
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_packed_rows");
}

int mvq_conv1d_vpacked_f32(const float* x, const float* wp, const float* bias, const float* residual, const float* alpha_out,
                           float* y, float* y2, const float* alpha2, int batch, int cin, int tin_rows, int tin_valid, int cout,
                           int ks, int stride, int dil, int pad, int act, int seg_per_row, int per_in, int tout_rows, void* stream)
{
    if (batch < 0 || cin <= 0 || cout <= 0 || ks <= 0 || stride <= 0 || dil <= 0 || pad < 0 || tin_rows <= 0 || tin_valid < 0 ||
        tin_valid > tin_rows || seg_per_row <= 0 || per_in <= 0 || tout_rows <= 0)
        return fail(MVQ_EINVAL, "conv1d_vpacked: bad shape");
    if (act != MVQ_ACT_NONE && act != MVQ_ACT_TANH && act != MVQ_ACT_GELU) return fail(MVQ_EINVAL, "conv1d_vpacked: bad act %d", act);
    const int tout = conv_out_len(tin_valid, ks, stride, dil, pad);             /* valid outputs per item */
    /* geometry of the virtual row: the output period is the physical output row, the input period is stride x that; between the
     * data of neighbouring items there must be at least `pad` zeros on the left and the last valid output's overhang on the right
     * (columns [tin_valid, tin_rows) of x are the caller's zero tail, columns beyond tin_rows come from the zero block) */
    const int per_out = tout_rows;
    const int overhang = (tout > 0 ? (tout - 1) * stride - pad + dil * (ks - 1) : 0) - (tin_valid - 1);   /* zeros needed behind the data */
    if (tin_rows % 4 != 0 || tout_rows % 4 != 0 || per_in % 4 != 0 || per_in != stride * per_out || tout > tout_rows ||
        tin_rows > per_in || per_in - tin_valid < pad || per_in - tin_valid < overhang)
        return fail(MVQ_EINVAL, "conv1d_vpacked: needs 16-byte rows, per_in == stride * tout_rows, tout <= tout_rows and a gap of at least "
                                "max(pad, overhang) zeros between items (tin_rows %d valid %d per_in %d tout %d tout_rows %d pad %d overhang %d)",
                    tin_rows, tin_valid, per_in, tout, tout_rows, pad, overhang);
    if ((long long)seg_per_row * per_in * per_in >= ((long long)1 << 32)) return fail(MVQ_EINVAL, "conv1d_vpacked: virtual row too long");
    if (batch == 0 || tout == 0) return MVQ_OK;
    if (!x || !wp || !y) return fail(MVQ_EINVAL, "conv1d_vpacked: null tensor");
    if ((y2 != nullptr) != (alpha2 != nullptr)) return fail(MVQ_EINVAL, "conv1d_vpacked: y2 and alpha2 go together");
    if (y2 && alpha_out) return fail(MVQ_EUNSUPPORTED, "conv1d_vpacked: a dual output and an output Snake together are not supported");
    mvq::ConvArgs a{};
    a.x = x; a.wp = wp; a.bias = bias; a.residual = residual; a.alpha_out = alpha_out; a.y = y; a.y2 = y2; a.alpha2 = alpha2;
    a.B = (batch + seg_per_row - 1) / seg_per_row;                               /* virtual rows */
    a.Cin = cin; a.Tin = seg_per_row * per_in; a.Cout = cout; a.Tout = tout_rows; a.pad = pad; a.Mpad = mvq::conv_mpad(cout);
    a.Mrows = cout; a.Ncols = seg_per_row * per_out; a.act = act; a.up_s = 1;
    a.vp_seg = seg_per_row; a.vp_per_in = per_in; a.vp_valid_in = tin_rows; a.vp_tin_phys = tin_rows; a.vp_btrue = batch;
    a.vp_per_out = per_out; a.vp_valid_out = tout; a.vp_magic_in = magic_div(per_in); a.vp_magic_out = magic_div(per_out);
    hipError_t e = dispatch_conv1d(a, ks, stride, dil, S(stream));
    if (e == hipErrorInvalidValue) return fail(MVQ_EUNSUPPORTED, "conv1d_vpacked: needs an MFMA-tiled, LDS-DMA-staged shape with the regular epilogue");
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_vpacked");
}

int mvq_conv_transpose1d_packed_rows_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                         const float* alpha_out, float* y, float* y2, const float* alpha2, int rows, int cin,
                                         int cout, int stride, int pad, int seg_per_row, int seg_period, int seg_valid,
                                         int batch_out, void* stream)
{
    if (rows < 0 || cin <= 0 || cout <= 0 || stride <= 0 || pad < 0 || seg_per_row <= 0 || seg_period <= 0 || seg_valid <= 0 || batch_out < 0)
        return fail(MVQ_EINVAL, "conv_transpose1d_packed_rows: bad shape");
    /* a segment's outputs must not reach into its neighbour's: the first `pad` positions are dropped, and the last outputs come
     * from input column seg_valid (a zero of the gap) -- which has to exist */
    if (seg_valid >= seg_period || batch_out > rows * seg_per_row)
        return fail(MVQ_EINVAL, "conv_transpose1d_packed_rows: needs at least one zero column between segments and rows * seg_per_row >= batch_out");
    const long long tin = (long long)seg_per_row * seg_period;
    const int tout = (seg_valid - 1) * stride - 2 * pad + 2 * stride;             /* per segment, as the unpacked layer gives */
    const long long per_out = (long long)seg_period * stride;
    if (tout <= 0 || tout > per_out) return fail(MVQ_EINVAL, "conv_transpose1d_packed_rows: bad segment length");
    if (tin * stride * per_out >= ((long long)1 << 32)) return fail(MVQ_EINVAL, "conv_transpose1d_packed_rows: row too long");
    if (rows == 0 || batch_out == 0) return MVQ_OK;
    if (!x || !wp || !y) return fail(MVQ_EINVAL, "conv_transpose1d_packed_rows: null tensor");
    if ((y2 != nullptr) != (alpha2 != nullptr)) return fail(MVQ_EINVAL, "conv_transpose1d_packed_rows: y2 and alpha2 go together");
    const int mrows = cout * stride;
    mvq::ConvArgs a{};
    a.x = x; a.wp = wp; a.bias = bias; a.alpha_in = alpha_in; a.alpha_out = alpha_out; a.y = y; a.y2 = y2; a.alpha2 = alpha2;
    a.B = rows; a.Cin = cin; a.Tin = (int)tin; a.Cout = cout; a.Tout = tout; a.pad = 1; a.Mpad = mvq::conv_mpad(mrows);
    a.Mrows = mrows; a.Ncols = (int)tin;          /* no boundary column: column tin would only feed positions past the last segment */
    a.up_s = stride; a.up_p = pad;
    a.up_per_out = (int)per_out; a.up_valid_out = tout; a.up_seg = seg_per_row; a.up_btrue = batch_out; a.up_magic = magic_div((int)per_out);
    hipError_t e = dispatch_convtr(a, S(stream));
    if (e == hipErrorInvalidValue) return fail(MVQ_EUNSUPPORTED, "conv_transpose1d_packed_rows: needs an MFMA-tiled shape");
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv_transpose1d_packed_rows");
}

static bool ru_fusable(int c, int dil)
{
    return (c == 64 || c == 96 || c == 128) && (dil == 1 || dil == 3 || dil == 9);
}

int mvq_residual_unit_kernel_name(int c, int dil, char* buf, int len)
{
    if (!buf || len <= 0) return fail(MVQ_EINVAL, "residual_unit_kernel_name: bad buffer");
    if (!ru_fusable(c, dil)) { snprintf(buf, len, "%s", "(two launches)"); return MVQ_OK; }
    mvq::ConvArgs a{};
    a.Cin = c; a.Cout = c; a.Mpad = mvq::conv_mpad(c); a.name_out = buf; a.name_len = len;
    (void)mvq::launch_residual_unit_fused(a, dil, nullptr);
    return MVQ_OK;
}

size_t mvq_residual_unit_scratch_floats(int batch, int c, int t, int dil)
{
    if (batch <= 0 || c <= 0 || t <= 0) return 0;
    return ru_fusable(c, dil) ? 0 : (size_t)batch * c * t;
}

int mvq_residual_unit_dual_f32(const float* x, const float* x_snaked, const float* w7p, const float* b7,
                               const float* alpha_a, const float* alpha_b, const float* w1p, const float* b1,
                               const float* alpha_next, float* y, float* y2, const float* alpha2, float* scratch,
                               int batch, int c, int t, int dil, void* stream);

int mvq_residual_unit_f32(const float* x, const float* w7p, const float* b7, const float* alpha_a,
                          const float* alpha_b, const float* w1p, const float* b1, const float* alpha_next,
                          float* y, float* scratch, int batch, int c, int t, int dil, void* stream)
{
    return mvq_residual_unit_dual_f32(x, nullptr, w7p, b7, alpha_a, alpha_b, w1p, b1, alpha_next, y, nullptr, nullptr,
                                      scratch, batch, c, t, dil, stream);
}

int mvq_residual_unit_dual_f32(const float* x, const float* x_snaked, const float* w7p, const float* b7,
                               const float* alpha_a, const float* alpha_b, const float* w1p, const float* b1,
                               const float* alpha_next, float* y, float* y2, const float* alpha2, float* scratch,
                               int batch, int c, int t, int dil, void* stream)
{
    return mvq_residual_unit_padded_f32(x, x_snaked, w7p, b7, alpha_a, alpha_b, w1p, b1, alpha_next, y, y2, alpha2, scratch,
                                        batch, c, t, dil, 0, stream);
}

int mvq_residual_unit_padded_f32(const float* x, const float* x_snaked, const float* w7p, const float* b7,
                                 const float* alpha_a, const float* alpha_b, const float* w1p, const float* b1,
                                 const float* alpha_next, float* y, float* y2, const float* alpha2, float* scratch,
                                 int batch, int c, int t, int dil, int tvalid, void* stream)
{
    if (batch < 0 || c <= 0 || t < 0 || dil <= 0) return fail(MVQ_EINVAL, "residual_unit: bad shape");
    if (tvalid < 0 || tvalid > t) return fail(MVQ_EINVAL, "residual_unit: tvalid outside [0, t]");
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!x || !w7p || !w1p || !alpha_a || !alpha_b || !y) return fail(MVQ_EINVAL, "residual_unit: null tensor");
    if ((y2 != nullptr) != (alpha2 != nullptr)) return fail(MVQ_EINVAL, "residual_unit: y2 and alpha2 go together");
    if (ru_fusable(c, dil)) {
        mvq::ConvArgs a{};
        /* x_snaked = snake_a(x) from the producer's dual output: the unit stages it as is (LDS-DMA ring, no Snake on load);
         * the skip path still adds the RAW x in the epilogue */
        a.x = x_snaked ? x_snaked : x; a.wp = w7p; a.bias = b7; a.alpha_in = x_snaked ? nullptr : alpha_a; a.residual = x;
        a.alpha_out = alpha_next; a.y = y;
        a.B = batch; a.Cin = c; a.Tin = t; a.Cout = c; a.Tout = t; a.pad = 3 * dil; a.Mpad = mvq::conv_mpad(c);
        a.Mrows = c; a.Ncols = t; a.act = 0; a.up_s = 1; a.up_p = 0;
        a.alpha_mid = alpha_b; a.w2p = w1p; a.bias2 = b1; a.y2 = y2; a.alpha2 = alpha2;
        a.tvalid = (tvalid == t) ? 0 : tvalid;
        hipError_t e = mvq::launch_residual_unit_fused(a, dil, S(stream));
        return e == hipSuccess ? MVQ_OK : hipfail(e, "residual_unit(fused)");
    }
    if (!scratch) return fail(MVQ_EINVAL, "residual_unit: scratch required for C=%d (see mvq_residual_unit_scratch_floats)", c);
    int rc = mvq_conv1d_padded_f32(x_snaked ? x_snaked : x, w7p, b7, x_snaked ? nullptr : alpha_a, nullptr, alpha_b, scratch,
                                   nullptr, nullptr, batch, c, t, c, 7, 1, dil, 3 * dil, MVQ_ACT_NONE, tvalid, stream);
    if (rc != MVQ_OK) return rc;
    return mvq_conv1d_padded_f32(scratch, w1p, b1, nullptr, x, alpha_next, y, y2, alpha2, batch, c, t, c, 1, 1, 1, 0,
                                 MVQ_ACT_NONE, tvalid, stream);
}

int mvq_conv_transpose1d_dual_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                  const float* alpha_out, float* y, float* y2, const float* alpha2,
                                  int batch, int cin, int tin, int cout, int stride, int pad, void* stream);

int mvq_conv_transpose1d_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                             const float* alpha_out, float* y,
                             int batch, int cin, int tin, int cout, int stride, int pad, void* stream)
{
    return mvq_conv_transpose1d_dual_f32(x, wp, bias, alpha_in, alpha_out, y, nullptr, nullptr, batch, cin, tin, cout, stride, pad, stream);
}

int mvq_conv_transpose1d_dual_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                  const float* alpha_out, float* y, float* y2, const float* alpha2,
                                  int batch, int cin, int tin, int cout, int stride, int pad, void* stream)
{
    return mvq_conv_transpose1d_padded_f32(x, wp, bias, alpha_in, alpha_out, y, y2, alpha2, batch, cin, tin, cout, stride, pad,
                                           0, 0, stream);
}

int mvq_conv_transpose1d_padded_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                    const float* alpha_out, float* y, float* y2, const float* alpha2,
                                    int batch, int cin, int tin, int cout, int stride, int pad, int tout_rows, int tvalid,
                                    void* stream)
{
    return mvq_conv_transpose1d_op_f32(x, wp, bias, alpha_in, alpha_out, y, y2, alpha2, batch, cin, tin, cout, stride, pad, 0,
                                       tout_rows, tvalid, stream);
}

int mvq_conv_transpose1d_op_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                const float* alpha_out, float* y, float* y2, const float* alpha2,
                                int batch, int cin, int tin, int cout, int stride, int pad, int output_padding, int tout_rows,
                                int tvalid, void* stream)
{
    if (batch < 0 || cin <= 0 || cout <= 0 || tin < 0 || stride <= 0 || pad < 0)
        return fail(MVQ_EINVAL, "conv_transpose1d: bad shape");
    /* torch: output_padding < stride; the polyphase form reaches `pad` columns past the un-padded length, so <= pad as well */
    if (output_padding < 0 || output_padding >= stride || output_padding > pad)
        return fail(MVQ_EINVAL, "conv_transpose1d: output_padding %d outside [0, min(stride - 1, pad)]", output_padding);
    const int tnat = (tin - 1) * stride - 2 * pad + 2 * stride + output_padding;
    /* tout_rows: length of the output rows (0 = the natural length).  Shorter than natural: the input carries a zero tail and
     * only its true outputs are wanted.  Up to `pad` longer (the polyphase form visits those columns too): rows padded to a
     * multiple of 4, columns >= tvalid zeroed. */
    const int tout = tout_rows > 0 ? tout_rows : tnat;
    if (tout > tnat - output_padding + pad || tvalid < 0 || tvalid > tout || (tout > tnat && (tvalid == 0 || tvalid > tnat)))
        return fail(MVQ_EINVAL, "conv_transpose1d: tout_rows %d / tvalid %d inconsistent with the natural length %d", tout, tvalid, tnat);
    if (batch == 0 || tin == 0 || tout <= 0) return MVQ_OK;
    if (!x || !wp || !y) return fail(MVQ_EINVAL, "conv_transpose1d: null tensor");
    if ((y2 != nullptr) != (alpha2 != nullptr)) return fail(MVQ_EINVAL, "conv_transpose1d: y2 and alpha2 go together");
    const int mrows = cout * stride;
    const int mpad = mvq::conv_mpad(mrows);
    hipError_t e;
    {
        mvq::ConvArgs a{};
        a.x = x; a.wp = wp; a.bias = bias; a.alpha_in = alpha_in; a.residual = nullptr; a.alpha_out = alpha_out; a.y = y;
        a.B = batch; a.Cin = cin; a.Tin = tin; a.Cout = cout; a.Tout = tout; a.pad = 1; a.Mpad = mpad;
        a.Mrows = mrows; a.Ncols = tin + 1; a.act = 0; a.up_s = stride; a.up_p = pad; a.y2 = y2; a.alpha2 = alpha2;
        a.tvalid = (tvalid == tout) ? 0 : tvalid;
        e = dispatch_convtr(a, S(stream));
    }
    if (e == hipErrorInvalidValue && (tvalid || tout_rows)) return fail(MVQ_EUNSUPPORTED, "conv_transpose1d: zero-padded rows need an MFMA-tiled shape");
    if (e == hipErrorInvalidValue) {
        (void)hipGetLastError();
        mvq::DirectConvArgs d{x, wp, bias, alpha_in, nullptr, alpha_out, y, batch, cin, tin, cout, tout, 2 * stride, stride, 1, pad, mpad, 0, y2, alpha2, nullptr, nullptr};
        e = mvq::launch_convtr_direct(d, S(stream));
    }
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv_transpose1d");
}

int mvq_rvq_ema_forward_f32(const float* z, const float* books, float* q_out, int32_t* idx_out,
                            int batch, int dim, int t, int nb_use, int k, void* stream)
{
    if (batch < 0 || t < 0 || dim <= 0 || dim > 128 || dim % 4 != 0 || nb_use < 0 || k <= 0)
        return fail(MVQ_EINVAL, "rvq_ema_forward: bad shape B=%d D=%d T=%d nb=%d K=%d", batch, dim, t, nb_use, k);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!z || !q_out || (nb_use > 0 && !books)) return fail(MVQ_EINVAL, "rvq_ema_forward: null tensor");
    hipError_t e = mvq::launch_rvq_ema_forward(z, books, q_out, idx_out, batch, dim, t, nb_use, k, 1, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "rvq_ema_forward");
}

size_t mvq_rvq_ema_step_scratch_bytes(int batch, int t, int nb, int k, int dim)
{
    if (batch <= 0 || t <= 0 || nb <= 0 || k <= 0 || dim <= 0) return 0;
    const size_t n = (size_t)batch * t;
    /* the per-book assignments, then the counting-sort workspace of the update (16-byte aligned) */
    return (((size_t)nb * n * sizeof(int32_t) + 15) & ~(size_t)15) + mvq::ema_update_scratch_bytes((int)n, nb, k, dim);
}

int mvq_rvq_ema_step_f32(const float* z_tokens, float* books, void* scratch,
                         int batch, int dim, int t, int nb, int k, float decay, void* stream)
{
    if (batch < 0 || t < 0 || dim <= 0 || dim > 128 || dim % 4 != 0 || nb <= 0 || k <= 0) return fail(MVQ_EINVAL, "rvq_ema_step: bad shape");
    if ((long long)batch * t >= (1ll << 24)) return fail(MVQ_EUNSUPPORTED, "rvq_ema_step: at most 2^24 - 1 tokens per call (counts are kept exact in fp32)");
    if (k > 16384) return fail(MVQ_EUNSUPPORTED, "rvq_ema_step: K <= 16384 (the per-segment histogram lives in LDS)");
    if (batch * t == 0) return MVQ_OK;
    if (!z_tokens || !books || !scratch) return fail(MVQ_EINVAL, "rvq_ema_step: null tensor");
    int32_t* idx = reinterpret_cast<int32_t*>(scratch);
    const size_t n = (size_t)batch * t;
    void* work = reinterpret_cast<char*>(scratch) + (((size_t)nb * n * sizeof(int32_t) + 15) & ~(size_t)15);
    hipError_t e = mvq::launch_rvq_ema_forward(z_tokens, books, nullptr, idx, batch, dim, t, nb, k, 0, S(stream));
    if (e != hipSuccess) return hipfail(e, "rvq_ema_step(assign)");
    e = mvq::launch_ema_update(z_tokens, idx, books, work, batch, dim, t, nb, k, decay, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "rvq_ema_step(update)");
}

int mvq_dac_rvq_f32(const float* z, const float* in_w, const float* in_b, const float* codebook,
                    const float* out_w, const float* out_b, float* zq, int32_t* codes, float* latents,
                    int batch, int c, int t, int nq_use, int k, int dc, void* stream)
{
    return mvq_dac_rvq_items_f32(z, in_w, in_b, codebook, out_w, out_b, zq, codes, latents, nullptr, batch, c, t, nq_use, k, dc, stream);
}

int mvq_dac_rvq_items_f32(const float* z, const float* in_w, const float* in_b, const float* codebook,
                          const float* out_w, const float* out_b, float* zq, int32_t* codes, float* latents,
                          const int32_t* nq_item, int batch, int c, int t, int nq_use, int k, int dc, void* stream)
{
    return mvq_dac_rvq_prepared_f32(z, in_w, in_b, codebook, nullptr, nullptr, out_w, out_b, zq, codes, latents, nq_item,
                                    batch, c, t, nq_use, k, dc, stream);
}

int mvq_rvq_dequant_f32(const int64_t* idx, const float* books, float* q_out, int batch, int dim, int t, int nb_use, int k,
                        size_t out_sb, size_t out_sd, void* stream)
{
    if (batch < 0 || t < 0 || dim <= 0 || dim % 4 != 0 || nb_use < 0 || k <= 0)
        return fail(MVQ_EINVAL, "rvq_dequant: bad shape B=%d D=%d T=%d nb=%d K=%d", batch, dim, t, nb_use, k);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!q_out || (nb_use > 0 && (!idx || !books))) return fail(MVQ_EINVAL, "rvq_dequant: null tensor");
    if (reinterpret_cast<uintptr_t>(books) & 15) return fail(MVQ_EINVAL, "rvq_dequant: books must be 16-byte aligned");
    if (out_sb == 0 && out_sd == 0) { out_sb = (size_t)dim * t; out_sd = (size_t)t; }
    hipError_t e = mvq::launch_rvq_dequant(idx, books, q_out, batch, dim, t, nb_use, k, out_sb, out_sd, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "rvq_dequant");
}

int mvq_dac_rvq_from_codes_f32(const int64_t* codes, const float* codebook, const float* out_w, const float* out_b, float* zq,
                               float* z_p, int batch, int c, int t, int nq_use, int k, int dc, void* stream)
{
    if (batch < 0 || t < 0 || c <= 0 || c % 64 != 0 || nq_use <= 0 || nq_use > 32 || k <= 0 || dc != 8)
        return fail(MVQ_EINVAL, "dac_rvq_from_codes: bad shape B=%d C=%d T=%d nq=%d K=%d Dc=%d (C %% 64 == 0, nq <= 32, Dc = 8)",
                    batch, c, t, nq_use, k, dc);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!codes || !codebook || !out_w || !out_b || !zq) return fail(MVQ_EINVAL, "dac_rvq_from_codes: null tensor");
    if ((reinterpret_cast<uintptr_t>(codebook) | reinterpret_cast<uintptr_t>(out_w)) & 15)
        return fail(MVQ_EINVAL, "dac_rvq_from_codes: codebook and out_w must be 16-byte aligned");
    hipError_t e = mvq::launch_dac_rvq_from_codes(codes, codebook, out_w, out_b, zq, z_p, batch, c, t, nq_use, k, dc, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "dac_rvq_from_codes");
}

int mvq_dac_rvq_from_codes_layers_f32(const int64_t* codes, size_t codes_sb, const float* codebook, const float* out_w, const float* out_b,
                                      const uint8_t* nq_valid, float* zq, float* z_p, int batch, int c, int t, int nq_use, int k, int dc,
                                      void* stream)
{
    if (!nq_valid && (codes_sb == 0 || codes_sb == (size_t)(nq_use > 0 ? nq_use : 0) * (size_t)(t > 0 ? t : 0)))
        return mvq_dac_rvq_from_codes_f32(codes, codebook, out_w, out_b, zq, z_p, batch, c, t, nq_use, k, dc, stream);
    if (batch < 0 || t < 0 || c <= 0 || c % 64 != 0 || nq_use <= 0 || nq_use > 32 || k <= 0 || dc != 8)
        return fail(MVQ_EINVAL, "dac_rvq_from_codes_layers: bad shape B=%d C=%d T=%d nq=%d K=%d Dc=%d (C %% 64 == 0, nq <= 32, Dc = 8)",
                    batch, c, t, nq_use, k, dc);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!nq_valid) return fail(MVQ_EINVAL, "dac_rvq_from_codes_layers: strided codes need nq_valid");
    if (!codes || !codebook || !out_w || !out_b || !zq) return fail(MVQ_EINVAL, "dac_rvq_from_codes_layers: null tensor");
    if ((reinterpret_cast<uintptr_t>(codebook) | reinterpret_cast<uintptr_t>(out_w)) & 15)
        return fail(MVQ_EINVAL, "dac_rvq_from_codes_layers: codebook and out_w must be 16-byte aligned");
    if (codes_sb == 0) codes_sb = (size_t)nq_use * t;
    if (codes_sb < (size_t)nq_use * t) return fail(MVQ_EINVAL, "dac_rvq_from_codes_layers: codes_sb is smaller than nq_use * T");
    hipError_t e = mvq::launch_dac_rvq_from_codes_layers(codes, codes_sb, codebook, out_w, out_b, nq_valid, zq, z_p, batch, c, t, nq_use, k,
                                                         dc, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "dac_rvq_from_codes_layers");
}

// ---- the lossy-channel receiver (kernels in packets.hip) ----
namespace {
// ceil(log2 K) when the packet kernels cover the shape (1..255 books and tokens per packet as the header holds them, at most 24
// bits per index), -1 otherwise.
inline int packet_bits(int batch, int nb, int t, int k, int packet_tok)
{
    if (batch < 0 || nb < 0 || nb > 255 || t < 0 || k < 1 || packet_tok < 1 || packet_tok > 255) return -1;
    int bits = 0;
    while (bits < 31 && (1u << bits) < (unsigned)k) ++bits;
    return bits <= 24 ? bits : -1;
}
}  // namespace

int mvq_idx_pack_packets_u8(const int64_t* idx, uint8_t* bodies, int batch, int nb, int t, int k, int packet_tok,
                            size_t s_book, size_t s_item, void* stream)
{
    const int bits = packet_bits(batch, nb, t, k, packet_tok);
    if (bits < 0)
        return fail(MVQ_EINVAL, "idx_pack_packets: bad shape B=%d nb=%d T=%d K=%d packet_tok=%d (nb, packet_tok <= 255, ceil(log2 K) <= 24)",
                    batch, nb, t, k, packet_tok);
    if (batch == 0 || t == 0 || nb == 0 || bits == 0) return MVQ_OK;          // no output byte
    if (!idx || !bodies) return fail(MVQ_EINVAL, "idx_pack_packets: null tensor");
    hipError_t e = mvq::launch_idx_pack_packets(idx, bodies, batch, nb, t, k, bits, packet_tok, s_book, s_item, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "idx_pack_packets");
}

int mvq_idx_unpack_packets(const uint8_t* bodies, const uint8_t* nb_recv, int64_t* idx, uint8_t* nb_valid, int batch, int nb, int t,
                           int k, int packet_tok, void* stream)
{
    const int bits = packet_bits(batch, nb, t, k, packet_tok);
    if (bits < 0)
        return fail(MVQ_EINVAL, "idx_unpack_packets: bad shape B=%d nb=%d T=%d K=%d packet_tok=%d (nb, packet_tok <= 255, ceil(log2 K) <= 24)",
                    batch, nb, t, k, packet_tok);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!nb_recv || !nb_valid || (nb > 0 && !idx) || (nb > 0 && bits > 0 && !bodies))
        return fail(MVQ_EINVAL, "idx_unpack_packets: null tensor");
    hipError_t e = mvq::launch_idx_unpack_packets(bodies, nb_recv, idx, nb_valid, batch, nb, t, k, bits, packet_tok, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "idx_unpack_packets");
}

// ---- forward error correction over the packet bodies: XOR parity and Reed-Solomon parity, r rows per group (kernels in fec.hip) ----
namespace {
// The shape checks of the FEC entry points: ceil(log2 K), or -1 with the message set.
inline int fec_bits(const char* who, int batch, int nb, int t, int k, int packet_tok, int group, int books)
{
    const int bits = packet_bits(batch, nb, t, k, packet_tok);
    if (bits < 0) {
        fail(MVQ_EINVAL, "%s: bad shape B=%d nb=%d T=%d K=%d packet_tok=%d (nb, packet_tok <= 255, ceil(log2 K) <= 24)", who, batch, nb, t, k,
             packet_tok);
        return -1;
    }
    if (group < 1 || group > 16 || books < 1 || books > nb) {
        fail(MVQ_EINVAL, "%s: bad shape group=%d (1..16) books=%d (1..nb=%d)", who, group, books, nb);
        return -1;
    }
    const long long P = ((long long)t + packet_tok - 1) / packet_tok;
    if ((long long)batch * ((P + group - 1) / group) > 2147483647LL) {
        fail(MVQ_EINVAL, "%s: bad shape B=%d x %lld parity groups exceed the grid", who, batch, (P + group - 1) / group);
        return -1;
    }
    return bits;
}

// The two bodies behind the four entry points: ``who`` is the name the messages print; the XOR entry points pass parity = 1 (which
// never fails the parity check) and got_any: any nonzero got byte says "arrived"; else got is a bitmask over the parity rows.
int fec_parity(const char* who, const uint8_t* bodies, const uint8_t* nb_sent, uint8_t* rows_out, int batch, int nb, int t, int k,
               int packet_tok, int group, int books, int parity, void* stream)
{
    const int bits = fec_bits(who, batch, nb, t, k, packet_tok, group, books);
    if (bits < 0) return MVQ_EINVAL;
    if (parity < 1 || parity > 4) return fail(MVQ_EINVAL, "%s: bad shape parity=%d (1..4)", who, parity);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!rows_out || (bits > 0 && !bodies)) return fail(MVQ_EINVAL, "%s: null tensor", who);
    hipError_t e = mvq::launch_fec_parity(bodies, nb_sent, rows_out, batch, nb, t, bits, packet_tok, group, books, parity, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, who);
}

int fec_recover(const char* who, uint8_t* bodies, uint8_t* nb_recv, const uint8_t* rows, const uint8_t* got, uint8_t* recovered, int batch,
                int nb, int t, int k, int packet_tok, int group, int books, int parity, bool got_any, void* stream)
{
    const int bits = fec_bits(who, batch, nb, t, k, packet_tok, group, books);
    if (bits < 0) return MVQ_EINVAL;
    if (parity < 1 || parity > 4) return fail(MVQ_EINVAL, "%s: bad shape parity=%d (1..4)", who, parity);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!nb_recv || !rows || !got || (bits > 0 && !bodies)) return fail(MVQ_EINVAL, "%s: null tensor", who);
    hipError_t e = mvq::launch_fec_recover(bodies, nb_recv, rows, got, recovered, batch, nb, t, bits, packet_tok, group, books, parity,
                                           got_any ? 0xffu : (1u << parity) - 1u, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, who);
}
}  // namespace

int mvq_fec_parity_u8(const uint8_t* bodies, const uint8_t* nb_sent, uint8_t* rows_out, int batch, int nb, int t, int k, int packet_tok,
                      int group, int books, void* stream)
{
    return fec_parity("fec_parity", bodies, nb_sent, rows_out, batch, nb, t, k, packet_tok, group, books, 1, stream);
}

int mvq_fec_recover_u8(uint8_t* bodies, uint8_t* nb_recv, const uint8_t* rows, const uint8_t* got, uint8_t* recovered, int batch, int nb,
                       int t, int k, int packet_tok, int group, int books, void* stream)
{
    return fec_recover("fec_recover", bodies, nb_recv, rows, got, recovered, batch, nb, t, k, packet_tok, group, books, 1, true, stream);
}

// Reed-Solomon parity, r rows per group: the XOR entry points' refusals, and parity outside 1..4; got is a bitmask over the r parities.
int mvq_fec_rs_parity_u8(const uint8_t* bodies, const uint8_t* nb_sent, uint8_t* rows_out, int batch, int nb, int t, int k,
                         int packet_tok, int group, int books, int parity, void* stream)
{
    return fec_parity("fec_rs_parity", bodies, nb_sent, rows_out, batch, nb, t, k, packet_tok, group, books, parity, stream);
}

int mvq_fec_rs_recover_u8(uint8_t* bodies, uint8_t* nb_recv, const uint8_t* rows, const uint8_t* got, uint8_t* recovered, int batch,
                          int nb, int t, int k, int packet_tok, int group, int books, int parity, void* stream)
{
    return fec_recover("fec_rs_recover", bodies, nb_recv, rows, got, recovered, batch, nb, t, k, packet_tok, group, books, parity,
                       false, stream);
}

int mvq_rvq_dequant_layers_f32(const int64_t* idx, const float* books, const uint8_t* nb_valid, float* q_out, int batch, int dim,
                               int t, int nb_use, int k, size_t out_sb, size_t out_sd, void* stream)
{
    if (!nb_valid) return mvq_rvq_dequant_f32(idx, books, q_out, batch, dim, t, nb_use, k, out_sb, out_sd, stream);
    if (batch < 0 || t < 0 || dim <= 0 || dim % 4 != 0 || nb_use < 0 || k <= 0)
        return fail(MVQ_EINVAL, "rvq_dequant_layers: bad shape B=%d D=%d T=%d nb=%d K=%d", batch, dim, t, nb_use, k);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!q_out || (nb_use > 0 && (!idx || !books))) return fail(MVQ_EINVAL, "rvq_dequant_layers: null tensor");
    if (reinterpret_cast<uintptr_t>(books) & 15) return fail(MVQ_EINVAL, "rvq_dequant_layers: books must be 16-byte aligned");
    if (out_sb == 0 && out_sd == 0) { out_sb = (size_t)dim * t; out_sd = (size_t)t; }
    hipError_t e = mvq::launch_rvq_dequant_layers(idx, books, nb_valid, q_out, batch, dim, t, nb_use, k, out_sb, out_sd, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "rvq_dequant_layers");
}

int mvq_dac_rvq_prepare_f32(const float* codebook, float* cb_normalised, float* cb_norm2, int nq, int k, int dc, void* stream)
{
    if (nq < 0 || k <= 0 || dc <= 0) return fail(MVQ_EINVAL, "dac_rvq_prepare: bad shape");
    if (nq == 0) return MVQ_OK;
    if (!codebook || !cb_normalised || !cb_norm2) return fail(MVQ_EINVAL, "dac_rvq_prepare: null tensor");
    hipError_t e = mvq::launch_dac_rvq_prepare(codebook, cb_normalised, cb_norm2, nq, k, dc, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "dac_rvq_prepare");
}

int mvq_dac_rvq_prepared_f32(const float* z, const float* in_w, const float* in_b, const float* codebook,
                             const float* cb_normalised, const float* cb_norm2,
                             const float* out_w, const float* out_b, float* zq, int32_t* codes, float* latents,
                             const int32_t* nq_item, int batch, int c, int t, int nq_use, int k, int dc, void* stream)
{
    if ((cb_normalised != nullptr) != (cb_norm2 != nullptr)) return fail(MVQ_EINVAL, "dac_rvq: cb_normalised and cb_norm2 go together");
    if (batch < 0 || t < 0 || (c != 1024 && c != 512 && c != 256) || dc != 8 || (k * dc) % 4 != 0 || nq_use <= 0 || k <= 0 || dc <= 0 || dc > 16)
        return fail(MVQ_EINVAL, "dac_rvq: bad shape B=%d C=%d T=%d nq=%d K=%d Dc=%d (C in {256,512,1024}, Dc = 8)", batch, c, t, nq_use, k, dc);
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!z || !zq || !codes || !latents || !in_w || !in_b || !codebook || !out_w || !out_b)
        return fail(MVQ_EINVAL, "dac_rvq: null tensor");
    const size_t lds = ((size_t)k * dc + k + (size_t)dc * c + 16 * (size_t)dc * 16 + 2 * (size_t)dc * 16 + 2 * 16 * 16) * sizeof(float);
    if (lds > 160 * 1024) return fail(MVQ_EUNSUPPORTED, "dac_rvq: K*Dc too large for LDS (%zu bytes)", lds);
    hipError_t e = mvq::launch_dac_rvq(z, in_w, in_b, codebook, out_w, out_b, zq, codes, latents, nq_item, batch, c, t, nq_use, k, dc, S(stream),
                                       cb_normalised, cb_norm2);
    return e == hipSuccess ? MVQ_OK : hipfail(e, "dac_rvq");
}

int mvq_layernorm_c_f32(const float* x, const float* pe, const float* gamma, const float* beta, float* y,
                        int batch, int c, int t, size_t stride_b, size_t stride_c,
                        float eps, int do_tanh, float post_scale, void* stream)
{
    return mvq_layernorm_c_sub_f32(x, nullptr, pe, gamma, beta, y, batch, c, t, stride_b, stride_c, eps, do_tanh, post_scale, stream);
}

int mvq_layernorm_c_sub_f32(const float* x, const float* sub, const float* pe, const float* gamma, const float* beta, float* y,
                            int batch, int c, int t, size_t stride_b, size_t stride_c,
                            float eps, int do_tanh, float post_scale, void* stream)
{
    if (c <= 0 || batch < 0 || t < 0) return fail(MVQ_EINVAL, "layernorm_c: bad shape");
    if (batch == 0 || t == 0) return MVQ_OK;                      /* empty chunk (Tk == 0 at a file end) */
    if (!x || !gamma || !beta || !y) return fail(MVQ_EINVAL, "layernorm_c: null tensor");
    if (stride_b == 0 && stride_c == 0) { stride_b = (size_t)c * t; stride_c = (size_t)t; }
    hipError_t e = mvq::launch_layernorm_c(x, pe, gamma, beta, y, batch, c, t, stride_b, stride_c, eps, do_tanh, post_scale, sub, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "layernorm_c");
}

int mvq_attention_f32(const float* q, const float* k, const float* v, float* ctx,
                      int batch, int heads, int dh, int tq, int tk,
                      size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, void* stream)
{
    if (batch < 0 || heads <= 0 || dh <= 0 || tq < 0 || tk < 0 || tk > 64 || tq > 64 || (size_t)dh * (tq + 2 * tk) + (size_t)tq * tk > 16384)
        return fail(MVQ_EINVAL, "attention: bad shape (Tq, Tk <= 64; head slices must fit 64 KiB of LDS)");
    if (batch == 0 || tq == 0) return MVQ_OK;
    if (!q || !ctx || (tk > 0 && (!k || !v))) return fail(MVQ_EINVAL, "attention: null tensor");
    const size_t c = (size_t)heads * dh;
    if (q_stride_b == 0 && q_stride_c == 0) { q_stride_b = c * tq; q_stride_c = (size_t)tq; }
    if (k_stride_b == 0 && k_stride_c == 0) { k_stride_b = c * tk; k_stride_c = (size_t)tk; }
    hipError_t e = mvq::launch_attention(q, k, v, ctx, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b, k_stride_c, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "attention");
}

int mvq_attention_masked_f32(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                             int batch, int heads, int dh, int tq, int tk,
                             size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, size_t m_stride_b, void* stream)
{
    if (!kmask || tk <= 0)                   /* NULL mask, or no key to mask: the existing launch and the existing bits */
        return mvq_attention_f32(q, k, v, ctx, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b, k_stride_c, stream);
    if (batch < 0 || heads <= 0 || dh <= 0 || tq < 0 || tk > 64 || tq > 64 || (size_t)dh * (tq + 2 * tk) + (size_t)tq * tk > 16384)
        return fail(MVQ_EINVAL, "attention_masked: bad shape (Tq, Tk <= 64; head slices must fit 64 KiB of LDS)");
    if (batch == 0 || tq == 0) return MVQ_OK;
    if (!q || !ctx || !k || !v) return fail(MVQ_EINVAL, "attention_masked: null tensor");
    const size_t c = (size_t)heads * dh;
    if (q_stride_b == 0 && q_stride_c == 0) { q_stride_b = c * tq; q_stride_c = (size_t)tq; }
    if (k_stride_b == 0 && k_stride_c == 0) { k_stride_b = c * tk; k_stride_c = (size_t)tk; }
    hipError_t e = mvq::launch_attention_masked(q, k, v, kmask, ctx, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b,
                                                k_stride_c, m_stride_b, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "attention_masked");
}

int mvq_hold_fill_f32(float* x, const uint8_t* valid, float* carry, int batch, int c, int t, void* stream)
{
    if (batch < 0 || c < 0 || t < 0 || (c + 15) / 16 > 65535) return fail(MVQ_EINVAL, "hold_fill: bad shape");
    if ((size_t)batch * c * t == 0) return MVQ_OK;
    if (!x || !valid) return fail(MVQ_EINVAL, "hold_fill: null tensor");
    hipError_t e = mvq::launch_hold_fill(x, valid, carry, batch, c, t, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "hold_fill");
}

int mvq_gelu_f32(const float* x, float* y, size_t n, void* stream)
{
    if ((!x || !y) && n) return fail(MVQ_EINVAL, "gelu: null tensor");
    hipError_t e = mvq::launch_gelu(x, y, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "gelu");
}

int mvq_sub3d_f32(const float* a, size_t a_sb, size_t a_sc, const float* b, size_t b_sb, size_t b_sc,
                  float* y, size_t y_sb, size_t y_sc, int batch, int c, int n, void* stream)
{
    if ((!a || !b || !y) && batch && c && n) return fail(MVQ_EINVAL, "sub3d: null tensor");
    if (batch < 0 || c < 0 || n < 0) return fail(MVQ_EINVAL, "sub3d: bad shape");
    hipError_t e = mvq::launch_strided3d(a, a_sb, a_sc, b, b_sb, b_sc, y, y_sb, y_sc, batch, c, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "sub3d");
}

int mvq_copy3d_f32(const float* a, size_t a_sb, size_t a_sc, float* y, size_t y_sb, size_t y_sc,
                   int batch, int c, int n, void* stream)
{
    if ((!a || !y) && batch && c && n) return fail(MVQ_EINVAL, "copy3d: null tensor");
    if (batch < 0 || c < 0 || n < 0) return fail(MVQ_EINVAL, "copy3d: bad shape");
    hipError_t e = mvq::launch_strided3d(a, a_sb, a_sc, nullptr, 0, 0, y, y_sb, y_sc, batch, c, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "copy3d");
}

int mvq_align_xcorr_f32(const float* ref, const float* est, int t, int max_shift, float* corr, int32_t* scratch,
                        int32_t* best_shift, void* stream)
{
    if (t < 0 || max_shift < 0) return fail(MVQ_EINVAL, "align_xcorr: bad shape");
    if (!ref || !est || !corr || !scratch || !best_shift) return fail(MVQ_EINVAL, "align_xcorr: null tensor");
    hipError_t e = mvq::launch_align_xcorr(ref, est, t, max_shift, corr, scratch, best_shift, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "align_xcorr");
}

int mvq_align_xcorr_batch_f32(const float* ref, const float* est, int batch, int t, int max_shift, float* corr, int32_t* scratch,
                              int32_t* best_shift, void* stream)
{
    if (batch < 0 || t < 0 || max_shift < 0) return fail(MVQ_EINVAL, "align_xcorr_batch: bad shape");
    if (batch == 0) return MVQ_OK;
    if (!ref || !est || !corr || !scratch || !best_shift) return fail(MVQ_EINVAL, "align_xcorr_batch: null tensor");
    hipError_t e = mvq::launch_align_xcorr_batch(ref, est, batch, t, max_shift, corr, scratch, best_shift, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "align_xcorr_batch");
}

int mvq_resample_ragged_f32(const float* x, const float* kern, float* y, const int32_t* off, const int32_t* len, int32_t* len_out,
                            int batch, int pitch, int lout_pitch, int orig, int newf, int width, int ks, void* stream)
{
    if (batch < 0 || pitch < 0 || lout_pitch < 0 || orig <= 0 || newf <= 0 || width < 0 || ks != 2 * width + orig)
        return fail(MVQ_EINVAL, "resample_ragged: bad shape (ks must be 2*width + orig)");
    /* off / len live on the device and cannot be checked here: the kernel clamps every slice to its row (off >= 0,
     * off + len <= pitch) and writes at most lout_pitch samples per row; len_out reports the length actually produced */
    if (batch == 0 || lout_pitch == 0) return MVQ_OK;
    if (!x || !kern || !y || !off || !len) return fail(MVQ_EINVAL, "resample_ragged: null tensor");
    hipError_t e = mvq::launch_resample_ragged(x, kern, y, off, len, len_out, batch, pitch, lout_pitch, orig, newf, width, ks, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "resample_ragged");
}

/* ---- backward (input-gradient) entry points: SURVEY.md section 8f row f1 ------------------------------------- */

size_t mvq_conv1d_dgrad_packed_floats(int cin, int cout, int ks)
{
    if (cin <= 0 || cout <= 0 || ks <= 0) return 0;
    return (size_t)cout * ks * mvq::conv_mpad(cin);
}

int mvq_conv1d_pack_dgrad_f32(const float* w, float* wp, int cin, int cout, int ks, void* stream)
{
    if (!w || !wp || cin <= 0 || cout <= 0 || ks <= 0) return fail(MVQ_EINVAL, "conv1d_pack_dgrad: bad argument");
    hipError_t e = mvq::launch_pack_conv1d_dgrad(w, wp, cin, cout, ks, mvq::conv_mpad(cin), S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_pack_dgrad");
}

int mvq_conv_transpose1d_pack_dgrad_f32(const float* w, float* wp, int cin, int cout, int ks, void* stream)
{
    if (!w || !wp || cin <= 0 || cout <= 0 || ks <= 0) return fail(MVQ_EINVAL, "conv_transpose1d_pack_dgrad: bad argument");
    hipError_t e = mvq::launch_pack_convtr_dgrad(w, wp, cin, cout, ks, mvq::conv_mpad(cin), S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv_transpose1d_pack_dgrad");
}

int mvq_conv1d_dgrad_f32(const float* gy, const float* wp_dgrad, const float* dsnake_src, const float* dsnake_alpha,
                         const float* residual, float* gx,
                         int batch, int cin, int tin, int cout, int tout, int ks, int stride, int dil, int pad, void* stream)
{
    /* gradient w.r.t. the input of a forward conv x[B,cin,tin] -> y[B,cout,tout]:
     *   stride 1 : conv1d over gy with the flipped/transposed image, same dilation, padding (ks-1)*dil - pad
     *   (forward was a ConvTranspose1d with kernel ks, stride, pad; its input-gradient is a strided conv): stride > 1 */
    if (batch < 0 || cin <= 0 || cout <= 0 || tin < 0 || tout < 0 || ks <= 0 || stride <= 0 || dil <= 0 || pad < 0)
        return fail(MVQ_EINVAL, "conv1d_dgrad: bad shape");
    if (batch == 0 || tin == 0) return MVQ_OK;
    if (!gy || !wp_dgrad || !gx) return fail(MVQ_EINVAL, "conv1d_dgrad: null tensor");
    if ((dsnake_src != nullptr) != (dsnake_alpha != nullptr)) return fail(MVQ_EINVAL, "conv1d_dgrad: dsnake_src and dsnake_alpha go together");
    const int bpad = stride == 1 ? (ks - 1) * dil - pad : pad;
    if (bpad < 0) return fail(MVQ_EUNSUPPORTED, "conv1d_dgrad: padding larger than the receptive field");
    const int olen = conv_out_len(tout, ks, stride, dil, bpad);
    if (olen != tin) return fail(MVQ_EINVAL, "conv1d_dgrad: shapes inconsistent (got %d input-gradient samples, expected %d)", olen, tin);
    mvq::ConvArgs a{};
    a.x = gy; a.wp = wp_dgrad; a.residual = residual; a.y = gx;
    a.B = batch; a.Cin = cout; a.Tin = tout; a.Cout = cin; a.Tout = tin; a.pad = bpad; a.Mpad = mvq::conv_mpad(cin);
    a.Mrows = cin; a.Ncols = tin; a.up_s = 1; a.dsn_src = dsnake_src; a.dsn_alpha = dsnake_alpha;
    hipError_t e = dispatch_conv1d(a, ks, stride, dil, S(stream));
    if (e == hipErrorInvalidValue) {
        (void)hipGetLastError();
        mvq::DirectConvArgs d{gy, wp_dgrad, nullptr, nullptr, residual, nullptr, gx, batch, cout, tout, cin, tin, ks, stride, dil, bpad,
                              a.Mpad, 0, nullptr, nullptr, dsnake_src, dsnake_alpha};
        e = mvq::launch_conv1d_direct(d, S(stream));
    }
    return e == hipSuccess ? MVQ_OK : hipfail(e, "conv1d_dgrad");
}

/* backward of the reference-owned trainable modules (tolerance-checked against torch autograd) */
int mvq_layernorm_c_bwd_f32(const float* x, const float* pe, const float* gamma, const float* g, float* gx,
                            float* dgamma, float* dbeta, float* stats, int batch, int c, int t,
                            size_t stride_b, size_t stride_c, float eps, void* stream)
{
    if (c <= 0 || batch < 0 || t < 0) return fail(MVQ_EINVAL, "layernorm_c_bwd: bad shape");
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!x || !gamma || !g || !dgamma || !dbeta || !stats) return fail(MVQ_EINVAL, "layernorm_c_bwd: null tensor");
    if (stride_b == 0 && stride_c == 0) { stride_b = (size_t)c * t; stride_c = (size_t)t; }
    hipError_t e = mvq::launch_layernorm_bwd(x, pe, gamma, g, gx, dgamma, dbeta, stats, batch, c, t, stride_b, stride_c, eps, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "layernorm_c_bwd");
}

int mvq_gelu_bwd_f32(const float* x, const float* g, float* gx, size_t n, void* stream)
{
    if ((!x || !g || !gx) && n) return fail(MVQ_EINVAL, "gelu_bwd: null tensor");
    hipError_t e = mvq::launch_gelu_bwd(x, g, gx, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "gelu_bwd");
}

int mvq_scale_tanh_f32(const float* u, float scale, float* y, size_t n, void* stream)
{
    if ((!u || !y) && n) return fail(MVQ_EINVAL, "scale_tanh: null tensor");
    hipError_t e = mvq::launch_scale_tanh(u, scale, y, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "scale_tanh");
}

int mvq_scale_tanh_bwd_f32(const float* u, const float* g, float scale, float* gu, float* partial, int n_partial, size_t n,
                           void* stream)
{
    if (((!u || !g || !gu) && n) || !partial || n_partial <= 0 || n_partial > 4096) return fail(MVQ_EINVAL, "scale_tanh_bwd: bad argument");
    hipError_t e = mvq::launch_scale_tanh_bwd(u, g, scale, gu, partial, n_partial, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "scale_tanh_bwd");
}

int mvq_attention_bwd_f32(const float* q, const float* k, const float* v, const float* g, float* gq, float* gk, float* gv,
                          int batch, int heads, int dh, int tq, int tk,
                          size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, void* stream)
{
    if (batch < 0 || heads <= 0 || dh <= 0 || tq < 0 || tk < 0 || tq > 32 || tk > 32) return fail(MVQ_EINVAL, "attention_bwd: bad shape (Tq, Tk <= 32)");
    if (batch == 0 || tq == 0) return MVQ_OK;
    if (!q || !g || !gq || (tk > 0 && (!k || !v || !gk || !gv))) return fail(MVQ_EINVAL, "attention_bwd: null tensor");
    const size_t c = (size_t)heads * dh;
    if (q_stride_b == 0 && q_stride_c == 0) { q_stride_b = c * tq; q_stride_c = (size_t)tq; }
    if (k_stride_b == 0 && k_stride_c == 0) { k_stride_b = c * tk; k_stride_c = (size_t)tk; }
    hipError_t e = mvq::launch_attention_bwd(q, k, v, g, gq, gk, gv, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b, k_stride_c, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "attention_bwd");
}

int mvq_attention_masked_bwd_f32(const float* q, const float* k, const float* v, const uint8_t* kmask, const float* g,
                                 float* gq, float* gk, float* gv, int batch, int heads, int dh, int tq, int tk,
                                 size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, size_t m_stride_b,
                                 void* stream)
{
    if (!kmask || tk <= 0)                   /* NULL mask, or no key to mask: the existing launch and the existing bits */
        return mvq_attention_bwd_f32(q, k, v, g, gq, gk, gv, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b, k_stride_c, stream);
    if (batch < 0 || heads <= 0 || dh <= 0 || tq < 0 || tq > 32 || tk > 32) return fail(MVQ_EINVAL, "attention_masked_bwd: bad shape (Tq, Tk <= 32)");
    if (((size_t)dh * (2 * tq + 2 * tk) + 2 * (size_t)tq * tk) * sizeof(float) > 64 * 1024)
        return fail(MVQ_EINVAL, "attention_masked_bwd: head slices must fit 64 KiB of LDS");
    if (batch == 0 || tq == 0) return MVQ_OK;
    if (!q || !g || !gq || !k || !v || !gk || !gv) return fail(MVQ_EINVAL, "attention_masked_bwd: null tensor");
    const size_t c = (size_t)heads * dh;
    if (q_stride_b == 0 && q_stride_c == 0) { q_stride_b = c * tq; q_stride_c = (size_t)tq; }
    if (k_stride_b == 0 && k_stride_c == 0) { k_stride_b = c * tk; k_stride_c = (size_t)tk; }
    hipError_t e = mvq::launch_attention_masked_bwd(q, k, v, kmask, g, gq, gk, gv, batch, heads, dh, tq, tk, q_stride_b, q_stride_c,
                                                    k_stride_b, k_stride_c, m_stride_b, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "attention_masked_bwd");
}

static const int kAttnSeqMaxT = 8192, kAttnSeqBwdMaxT = 512, kAttnSeqBwdMaxDh = 256;

int mvq_attention_seq_f32(const float* q, const float* k, const float* v, float* ctx,
                          int batch, int heads, int dh, int tq, int tk,
                          size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, void* stream)
{
    if (batch < 0 || heads <= 0 || dh <= 0 || tq < 0 || tk < 0 || tq > kAttnSeqMaxT || tk > kAttnSeqMaxT)
        return fail(MVQ_EINVAL, "attention_seq: bad shape (Tq, Tk <= %d)", kAttnSeqMaxT);
    int qt = 0, kt = 0;
    size_t nf = 0;
    if (!mvq::attn_seq_plan(dh, tk, &qt, &kt, &nf)) return fail(MVQ_EINVAL, "attention_seq: dh = %d does not fit a query tile in LDS", dh);
    if (batch == 0 || tq == 0) return MVQ_OK;
    if (!q || !ctx || (tk > 0 && (!k || !v))) return fail(MVQ_EINVAL, "attention_seq: null tensor");
    const size_t c = (size_t)heads * dh;
    if (q_stride_b == 0 && q_stride_c == 0) { q_stride_b = c * tq; q_stride_c = (size_t)tq; }
    if (k_stride_b == 0 && k_stride_c == 0) { k_stride_b = c * tk; k_stride_c = (size_t)tk; }
    hipError_t e = mvq::launch_attention_seq(q, k, v, ctx, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b, k_stride_c, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "attention_seq");
}

int mvq_attention_seq_masked_f32(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                                 int batch, int heads, int dh, int tq, int tk,
                                 size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, size_t m_stride_b, void* stream)
{
    if (!kmask || tk <= 0)                   /* NULL mask, or no key to mask: the existing launch and the existing bits */
        return mvq_attention_seq_f32(q, k, v, ctx, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b, k_stride_c, stream);
    if (batch < 0 || heads <= 0 || dh <= 0 || tq < 0 || tq > kAttnSeqMaxT || tk > kAttnSeqMaxT)
        return fail(MVQ_EINVAL, "attention_seq_masked: bad shape (Tq, Tk <= %d)", kAttnSeqMaxT);
    int qt = 0, kt = 0;
    size_t nf = 0;
    if (!mvq::attn_seq_plan(dh, tk, &qt, &kt, &nf)) return fail(MVQ_EINVAL, "attention_seq_masked: dh = %d does not fit a query tile in LDS", dh);
    if (batch == 0 || tq == 0) return MVQ_OK;
    if (!q || !ctx || !k || !v) return fail(MVQ_EINVAL, "attention_seq_masked: null tensor");
    const size_t c = (size_t)heads * dh;
    if (q_stride_b == 0 && q_stride_c == 0) { q_stride_b = c * tq; q_stride_c = (size_t)tq; }
    if (k_stride_b == 0 && k_stride_c == 0) { k_stride_b = c * tk; k_stride_c = (size_t)tk; }
    hipError_t e = mvq::launch_attention_seq_masked(q, k, v, kmask, ctx, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b,
                                                    k_stride_c, m_stride_b, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "attention_seq_masked");
}

size_t mvq_attention_seq_bwd_scratch_bytes(int batch, int heads, int tq, int tk)
{
    if (batch <= 0 || heads <= 0 || tq <= 0 || tk <= 0) return 0;
    return (size_t)2 * batch * heads * (size_t)tq * tk * sizeof(float);
}

int mvq_attention_seq_bwd_f32(const float* q, const float* k, const float* v, const float* g, float* gq, float* gk, float* gv,
                              void* scratch, int batch, int heads, int dh, int tq, int tk,
                              size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, void* stream)
{
    if (batch < 0 || heads <= 0 || dh <= 0 || dh > kAttnSeqBwdMaxDh || tq < 0 || tk < 0 || tq > kAttnSeqBwdMaxT || tk > kAttnSeqBwdMaxT)
        return fail(MVQ_EINVAL, "attention_seq_bwd: bad shape (Tq, Tk <= %d, dh <= %d)", kAttnSeqBwdMaxT, kAttnSeqBwdMaxDh);
    if (batch == 0 || tq == 0) return MVQ_OK;
    if (!q || !g || !gq || (tk > 0 && (!k || !v || !gk || !gv || !scratch))) return fail(MVQ_EINVAL, "attention_seq_bwd: null tensor");
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return fail(MVQ_EINVAL, "attention_seq_bwd: scratch must be 16-byte aligned");
    const size_t c = (size_t)heads * dh;
    if (q_stride_b == 0 && q_stride_c == 0) { q_stride_b = c * tq; q_stride_c = (size_t)tq; }
    if (k_stride_b == 0 && k_stride_c == 0) { k_stride_b = c * tk; k_stride_c = (size_t)tk; }
    hipError_t e = mvq::launch_attention_seq_bwd(q, k, v, g, gq, gk, gv, static_cast<float*>(scratch), batch, heads, dh, tq, tk,
                                                 q_stride_b, q_stride_c, k_stride_b, k_stride_c, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "attention_seq_bwd");
}

int mvq_attention_seq_masked_bwd_f32(const float* q, const float* k, const float* v, const uint8_t* kmask, const float* g,
                                     float* gq, float* gk, float* gv, void* scratch, int batch, int heads, int dh, int tq, int tk,
                                     size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c,
                                     size_t m_stride_b, void* stream)
{
    if (!kmask || tk <= 0)                   /* NULL mask, or no key to mask: the existing launch and the existing bits */
        return mvq_attention_seq_bwd_f32(q, k, v, g, gq, gk, gv, scratch, batch, heads, dh, tq, tk, q_stride_b, q_stride_c, k_stride_b,
                                         k_stride_c, stream);
    if (batch < 0 || heads <= 0 || dh <= 0 || dh > kAttnSeqBwdMaxDh || tq < 0 || tq > kAttnSeqBwdMaxT || tk > kAttnSeqBwdMaxT)
        return fail(MVQ_EINVAL, "attention_seq_masked_bwd: bad shape (Tq, Tk <= %d, dh <= %d)", kAttnSeqBwdMaxT, kAttnSeqBwdMaxDh);
    if (batch == 0 || tq == 0) return MVQ_OK;
    if (!q || !g || !gq || !k || !v || !gk || !gv || !scratch) return fail(MVQ_EINVAL, "attention_seq_masked_bwd: null tensor");
    if (reinterpret_cast<uintptr_t>(scratch) % 16) return fail(MVQ_EINVAL, "attention_seq_masked_bwd: scratch must be 16-byte aligned");
    const size_t c = (size_t)heads * dh;
    if (q_stride_b == 0 && q_stride_c == 0) { q_stride_b = c * tq; q_stride_c = (size_t)tq; }
    if (k_stride_b == 0 && k_stride_c == 0) { k_stride_b = c * tk; k_stride_c = (size_t)tk; }
    hipError_t e = mvq::launch_attention_seq_masked_bwd(q, k, v, kmask, g, gq, gk, gv, static_cast<float*>(scratch), batch, heads, dh,
                                                        tq, tk, q_stride_b, q_stride_c, k_stride_b, k_stride_c, m_stride_b, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "attention_seq_masked_bwd");
}

static inline uint32_t chan_fold_host(uint32_t h, uint32_t f)
{
    uint32_t x = (h ^ f) + 0x9e3779b9u;
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}

int mvq_channel_draw_u8(uint8_t* counts, int batch, int t, int packet_tok, int nb, int min_books,
                        uint64_t thr_loss, uint64_t thr_thin, uint64_t thr_gb, uint64_t thr_bg, uint64_t thr_loss_bad,
                        uint32_t seed, uint32_t step, uint32_t stream_id, uint32_t item_base, void* stream)
{
    const uint64_t one = (uint64_t)1 << 32;
    if (batch < 0 || t < 0 || packet_tok <= 0 || nb < 1 || nb > 255 || min_books < 1 || min_books > nb)
        return fail(MVQ_EINVAL, "channel_draw: bad shape (packet_tok >= 1, 1 <= min_books <= nb <= 255)");
    if (thr_loss > one || thr_thin > one || thr_gb > one || thr_bg > one || thr_loss_bad > one)
        return fail(MVQ_EINVAL, "channel_draw: a threshold above 2^32");
    if (batch == 0 || t == 0) return MVQ_OK;
    if (!counts) return fail(MVQ_EINVAL, "channel_draw: null tensor");
    const uint32_t hs = chan_fold_host(chan_fold_host(chan_fold_host(0u, seed), step), stream_id);
    hipError_t e = mvq::launch_channel_draw(counts, batch, t, packet_tok, nb, min_books, thr_loss, thr_thin, thr_gb, thr_bg,
                                            thr_loss_bad, hs, item_base, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "channel_draw");
}

int mvq_plc_mask_fill_f32(const float* zt, const float* z_pred, const uint8_t* mask, float* zt_in, float* z_filled,
                          int batch, int c, int t, size_t stride_b, size_t stride_c, void* stream)
{
    if (batch < 0 || c < 0 || t < 0) return fail(MVQ_EINVAL, "plc_mask_fill: bad shape");
    if ((size_t)batch * c * t == 0) return MVQ_OK;
    if (!zt || !mask || (!zt_in && !z_filled) || (z_filled && !z_pred)) return fail(MVQ_EINVAL, "plc_mask_fill: null tensor");
    if (stride_b == 0 && stride_c == 0) { stride_b = (size_t)c * t; stride_c = (size_t)t; }
    hipError_t e = mvq::launch_plc_mask_fill(zt, z_pred, mask, zt_in, z_filled, batch, c, t, stride_b, stride_c, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "plc_mask_fill");
}

int mvq_plc_mask_fill_bwd_f32(const float* g, const uint8_t* mask, float* g_zpred,
                              int batch, int c, int t, size_t stride_b, size_t stride_c, void* stream)
{
    if (batch < 0 || c < 0 || t < 0) return fail(MVQ_EINVAL, "plc_mask_fill_bwd: bad shape");
    if ((size_t)batch * c * t == 0) return MVQ_OK;
    if (!g || !mask || !g_zpred) return fail(MVQ_EINVAL, "plc_mask_fill_bwd: null tensor");
    if (stride_b == 0 && stride_c == 0) { stride_b = (size_t)c * t; stride_c = (size_t)t; }
    hipError_t e = mvq::launch_plc_mask_fill_bwd(g, mask, g_zpred, batch, c, t, stride_b, stride_c, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "plc_mask_fill_bwd");
}

static const int kMelSsimMaxWidth = 32768, kMelRows = 64, kSubsetMaxT = 1 << 24;

int mvq_frame_subsets(const uint8_t* latent_mask, int t_lat, long long t_wave, int hop, int t_frames, uint8_t* frame_mask,
                      int* cols_masked, int* cols_unmasked, int* counts, void* stream)
{
    if (t_lat < 0 || t_wave < 0 || hop <= 0 || t_frames < 0 || t_frames > kMelSsimMaxWidth)
        return fail(MVQ_EINVAL, "frame_subsets: bad shape (0 <= frames <= %d, hop > 0)", kMelSsimMaxWidth);
    if (!counts || (t_frames > 0 && (!frame_mask || !cols_masked || !cols_unmasked)) || (t_lat > 0 && !latent_mask))
        return fail(MVQ_EINVAL, "frame_subsets: null tensor");
    const double spt = (t_lat > 0 && t_wave > 0) ? (double)t_wave / (double)t_lat : 0.0;
    hipError_t e = mvq::launch_frame_subsets(latent_mask, spt > 0.0 ? t_lat : 0, spt, hop, t_frames, frame_mask, cols_masked,
                                             cols_unmasked, counts, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "frame_subsets");
}

int mvq_mel_ssim_f32(const float* mel, int rows, size_t ld, const float* maxv, int n_maxv, const int* desc, const int* cols,
                     size_t n_cols, const int* widths, int n, int max_width, int mode, double* out, void* stream)
{
    if (rows != kMelRows) return fail(MVQ_EINVAL, "mel_ssim: rows = %d (the mel front end has %d)", rows, kMelRows);
    if (n < 0 || max_width < 0 || max_width > kMelSsimMaxWidth || (size_t)max_width > ld || ld > (size_t)1 << 30)
        return fail(MVQ_EINVAL, "mel_ssim: bad shape (width <= %d and <= ld)", kMelSsimMaxWidth);
    if (mode != MVQ_SSIM_NORM && mode != MVQ_SSIM_SSIM) return fail(MVQ_EINVAL, "mel_ssim: unknown mode %d", mode);
    if (n == 0) return MVQ_OK;
    if (!mel || !maxv || n_maxv <= 0 || !desc || !widths || !out || (n_cols > 0 && !cols)) return fail(MVQ_EINVAL, "mel_ssim: null tensor");
    hipError_t e = mvq::launch_mel_ssim(mel, ld, maxv, n_maxv, desc, cols, n_cols, widths, n, max_width, mode, out, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "mel_ssim");
}

int mvq_subset_stats_f32(const float* ref, const float* est, long long t, const uint8_t* latent_mask, int t_lat, double* out,
                         void* stream)
{
    if (t < 0 || t > kSubsetMaxT || t_lat < 0) return fail(MVQ_EINVAL, "subset_stats: bad shape (0 <= T <= %d)", kSubsetMaxT);
    if (!out || (t > 0 && (!ref || !est)) || (t_lat > 0 && !latent_mask)) return fail(MVQ_EINVAL, "subset_stats: null tensor");
    const float spt = (t_lat > 0 && t > 0) ? (float)((double)t / (double)t_lat) : 1.0f;
    hipError_t e = mvq::launch_subset_stats(ref, est, (int)t, latent_mask, t > 0 ? t_lat : 0, spt, out, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "subset_stats");
}

int mvq_mul_scaled_f32(const float* a, const float* b, float scale, float* out, size_t n, void* stream)
{
    if ((!a || !b || !out) && n) return fail(MVQ_EINVAL, "mul_scaled: null tensor");
    hipError_t e = mvq::launch_mul_scaled(a, b, scale, out, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "mul_scaled");
}

int mvq_transpose2d_f32(const float* in, float* out, int rows, int cols, void* stream)
{
    if (rows < 0 || cols < 0) return fail(MVQ_EINVAL, "transpose2d: bad shape");
    if ((!in || !out) && rows && cols) return fail(MVQ_EINVAL, "transpose2d: null tensor");
    hipError_t e = mvq::launch_transpose2d(in, out, rows, cols, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "transpose2d");
}

int mvq_rowsum_f32(const float* in, float* out, int rows, int cols, int accumulate, void* stream)
{
    if (rows < 0 || cols < 0) return fail(MVQ_EINVAL, "rowsum: bad shape");
    if ((!in && rows && cols) || (!out && rows)) return fail(MVQ_EINVAL, "rowsum: null tensor");   /* cols == 0: nothing is read, out = 0 */
    hipError_t e = mvq::launch_rowsum(in, out, rows, cols, accumulate, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "rowsum");
}

/* training losses (row f2): the glue kernels around the STFT-as-GEMM; see include/mvq.h */
#define MVQ_LOSS_CALL(cond, what, call) do { if (cond) return fail(MVQ_EINVAL, what ": bad argument"); \
    hipError_t e_ = (call); return e_ == hipSuccess ? MVQ_OK : hipfail(e_, what); } while (0)

int mvq_stft_frames_f32(const float* x, const float* window, float* out, int batch, int t, int n_fft, int hop, int nframes,
                        size_t ncols, size_t col0, void* stream)
{
    MVQ_LOSS_CALL(!x || !window || !out || batch < 0 || t <= n_fft / 2 || n_fft <= 0 || hop <= 0 || nframes != 1 + t / hop ||
                  col0 + (size_t)batch * nframes > ncols, "stft_frames",
                  mvq::launch_stft_frames(x, window, out, batch, t, n_fft, hop, nframes, ncols, col0, S(stream)));
}
int mvq_spec_mag_f32(const float* spec, float* mag, int f, int fp, size_t ncols, float eps, void* stream)
{
    MVQ_LOSS_CALL(!spec || !mag || f <= 0 || fp < f, "spec_mag", mvq::launch_spec_mag(spec, mag, f, fp, ncols, eps, S(stream)));
}
int mvq_spec_loss_partial_f32(const float* mag, float* partial, int p, int f, int batch, int nframes, size_t ncols, void* stream)
{
    MVQ_LOSS_CALL(!mag || !partial || p <= 0 || f <= 0 || batch < 0 || (size_t)2 * batch * nframes > ncols, "spec_loss_partial",
                  mvq::launch_spec_loss_partial(mag, partial, p, f, batch, nframes, ncols, S(stream)));
}
int mvq_spec_grad_f32(const float* spec, const float* mag, const float* coef_a, float coef_b, const float* extra, float* g,
                      int f, int fp, int batch, int nframes, size_t ncols, float eps, void* stream)
{
    MVQ_LOSS_CALL(!spec || !mag || !g || f <= 0 || fp < f || batch < 0 || (size_t)2 * batch * nframes > ncols, "spec_grad",
                  mvq::launch_spec_grad(spec, mag, coef_a, coef_b, extra, g, f, fp, batch, nframes, ncols, eps, S(stream)));
}
int mvq_overlap_add_f32(const float* dframes, const float* window, float* dy, int batch, int t, int n_fft, int hop, int nframes,
                        void* stream)
{
    MVQ_LOSS_CALL(!dframes || !window || !dy || batch < 0 || t <= n_fft / 2 || hop <= 0 || nframes != 1 + t / hop, "overlap_add",
                  mvq::launch_overlap_add(dframes, window, dy, batch, t, n_fft, hop, nframes, S(stream)));
}
int mvq_l1_loss_f32(const float* y, const float* tgt, float* partial, int p, float* dy, float coef, size_t n, void* stream)
{
    MVQ_LOSS_CALL(!y || !tgt || !partial || p <= 0 || p > 4096, "l1_loss", mvq::launch_l1_loss(y, tgt, partial, p, dy, coef, n, S(stream)));
}
int mvq_mel_max_f32(const float* mel, float* maxv, int* argmax, int n_mels, int batch, int nframes, size_t ncols, void* stream)
{
    MVQ_LOSS_CALL(!mel || !maxv || !argmax || n_mels <= 0 || batch < 0 || (size_t)2 * batch * nframes > ncols, "mel_max",
                  mvq::launch_mel_max(mel, maxv, argmax, n_mels, batch, nframes, ncols, S(stream)));
}
int mvq_mel_cos_f32(const float* mel, const float* maxv, float* cosv, float* dmel, float* dden, float coef, int n_mels, int batch,
                    int nframes, size_t ncols, float eps, int use_log, void* stream)
{
    MVQ_LOSS_CALL(!mel || !maxv || !cosv || (dmel && (!dden || !use_log)) || n_mels <= 0 || batch < 0 || (size_t)2 * batch * nframes > ncols, "mel_cos",
                  mvq::launch_mel_cos(mel, maxv, cosv, dmel, dden, coef, n_mels, batch, nframes, ncols, eps, use_log, S(stream)));
}
int mvq_mel_max_grad_f32(const float* dden, const float* maxv, const int* argmax, float* dmel, int batch, int nframes, float eps,
                         void* stream)
{
    MVQ_LOSS_CALL(!dden || !maxv || !argmax || !dmel || batch < 0, "mel_max_grad",
                  mvq::launch_mel_max_grad(dden, maxv, argmax, dmel, batch, nframes, eps, S(stream)));
}

int mvq_resample_f32(const float* x, const float* kern, float* y, int batch, int len, int len_out, int orig, int newf,
                     int width, int ks, void* stream)
{
    if (batch < 0 || len < 0 || len_out < 0 || orig <= 0 || newf <= 0 || width < 0 || ks != 2 * width + orig)
        return fail(MVQ_EINVAL, "resample: bad shape (ks must be 2*width + orig)");
    if ((long long)len_out > ((long long)newf * len + orig - 1) / orig) return fail(MVQ_EINVAL, "resample: len_out exceeds ceil(new*len/orig)");
    if (batch == 0 || len_out == 0) return MVQ_OK;
    if (!x || !kern || !y) return fail(MVQ_EINVAL, "resample: null tensor");
    hipError_t e = mvq::launch_resample(x, kern, y, batch, len, len_out, orig, newf, width, ks, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "resample");
}

// ---- the streaming state kernels: dense sessions, and slots[n_group] of a pool of n_slots sessions ----
static int slots_shape_bad(const char* who, int n_group, int n_slots, long long per_session)
{
    if (n_group < 0 || n_slots < 0) return fail(MVQ_EINVAL, "%s: negative size", who);
    if (n_group > n_slots) return fail(MVQ_EINVAL, "%s: a group of %d sessions in a pool of %d slots", who, n_group, n_slots);
    if ((long long)n_group * per_session > 0x7FFFFFFFLL) return fail(MVQ_EINVAL, "%s: %d sessions of %lld rows", who, n_group, per_session);
    return MVQ_OK;
}

// The one argument check of the streamed resampler (`who`: the entry point) -> the launch's state length, output count, base, lead.
struct ResampleStreamPlan { int ns, n_out, base, lead; };
static int resample_stream_plan(const char* who, int batch, int n_new, long long consumed, int final, int len_out, int orig, int newf,
                                int width, int ks, ResampleStreamPlan* p)
{
    if (batch < 0 || n_new < 0 || consumed < 0 || len_out < 0 || orig <= 0 || newf <= 0 || width < 0 || ks != 2 * width + orig)
        return fail(MVQ_EINVAL, "%s: bad shape (ks must be 2*width + orig)", who);
    if (newf != 1) return fail(MVQ_EUNSUPPORTED, "%s: pure decimation only (newf = %d after the gcd)", who, newf);
    const long long hold = (width + orig - 1) / orig;
    const long long ns = hold * orig + width;
    if (ns > 1024) return fail(MVQ_EUNSUPPORTED, "%s: state of %lld samples exceeds 1024", who, ns);
    if (consumed % orig) return fail(MVQ_EINVAL, "%s: consumed = %lld is no multiple of orig = %d", who, consumed, orig);
    if (!final && n_new % orig)
        return fail(MVQ_EINVAL, "%s: n_new = %d is no multiple of orig = %d (only the final call may be)", who, n_new, orig);
    const long long q0 = consumed / orig;
    const long long done = q0 > hold ? q0 - hold : 0;
    const long long q1 = final ? (consumed + n_new + orig - 1) / orig : q0 + n_new / orig - hold;
    const long long n_out = q1 > done ? q1 - done : 0;
    if (n_out != len_out) return fail(MVQ_EINVAL, "%s: len_out = %d, this call completes %lld outputs", who, len_out, n_out);
    const int base = (int)(q0 < hold ? (hold - q0) * orig : 0);
    const int lead = (int)(consumed < ns ? ns - consumed : 0);
    *p = {(int)ns, (int)n_out, base, lead};
    return MVQ_OK;
}

int mvq_resample_stream_f32(const float* x_new, const float* kern, float* state, float* y, int batch, int n_new, long long consumed,
                            int final, int len_out, int orig, int newf, int width, int ks, void* stream)
{
    ResampleStreamPlan p;
    if (int rc = resample_stream_plan("resample_stream", batch, n_new, consumed, final, len_out, orig, newf, width, ks, &p)) return rc;
    if (batch == 0) return MVQ_OK;
    if (!kern || !state || (!x_new && n_new) || (!y && p.n_out)) return fail(MVQ_EINVAL, "resample_stream: null tensor");
    hipError_t e = mvq::launch_resample_stream(x_new, kern, state, nullptr, y, batch, n_new, p.n_out, orig, ks, p.ns, p.base, p.lead, 0,
                                               S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "resample_stream");
}

int mvq_resample_stream_slots_f32(const float* x_new, const float* kern, float* state, const int32_t* slots, int n_group, int n_slots,
                                  float* y, int n_new, long long consumed, int final, int len_out, int orig, int newf, int width, int ks,
                                  void* stream)
{
    if (int rc = slots_shape_bad("resample_stream_slots", n_group, n_slots, 1)) return rc;
    ResampleStreamPlan p;
    if (int rc = resample_stream_plan("resample_stream_slots", n_group, n_new, consumed, final, len_out, orig, newf, width, ks, &p)) return rc;
    if (consumed && consumed < p.ns)
        return fail(MVQ_EINVAL, "resample_stream_slots: consumed = %lld inside the %d-sample state names no launch class (0, or at least %d)",
                    consumed, p.ns, p.ns);
    if ((long long)n_group * p.n_out > 0x7FFFFFFFLL) return fail(MVQ_EINVAL, "resample_stream_slots: %d x %d outputs", n_group, p.n_out);
    if (n_group == 0) return MVQ_OK;
    if (!kern || !state || !slots || (!x_new && n_new) || (!y && p.n_out)) return fail(MVQ_EINVAL, "resample_stream_slots: null tensor");
    hipError_t e = mvq::launch_resample_stream(x_new, kern, state, slots, y, n_group, n_new, p.n_out, orig, ks, p.ns, p.base, p.lead,
                                               n_slots, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "resample_stream_slots");
}

// The one argument check of the rational streamed resampler: resample_stream_plan with a bank of newf phases and the lag `hold`
// (in blocks of orig inputs / newf outputs) chosen by the caller.
static int resample_rational_plan(const char* who, int batch, int n_new, long long consumed, int final, int len_out, int orig, int newf,
                                  int width, int ks, int hold, ResampleStreamPlan* p)
{
    if (batch < 0 || n_new < 0 || consumed < 0 || len_out < 0 || orig <= 0 || newf <= 0 || width < 0 || hold < 0 || ks != 2 * width + orig)
        return fail(MVQ_EINVAL, "%s: bad shape (ks must be 2*width + orig)", who);
    if (consumed > (1LL << 40)) return fail(MVQ_EINVAL, "%s: consumed = %lld", who, consumed);
    if (hold < (width + orig - 1) / orig)
        return fail(MVQ_EINVAL, "%s: hold = %d blocks is less than ceil(width/orig) = %d", who, hold, (width + orig - 1) / orig);
    const long long ns = (long long)hold * orig + width;
    if (ns > 1024) return fail(MVQ_EUNSUPPORTED, "%s: state of %lld samples exceeds 1024", who, ns);
    if (consumed % orig) return fail(MVQ_EINVAL, "%s: consumed = %lld is no multiple of orig = %d", who, consumed, orig);
    if (!final && n_new % orig)
        return fail(MVQ_EINVAL, "%s: n_new = %d is no multiple of orig = %d (only the final call may be)", who, n_new, orig);
    if (ns + n_new > 0x7FFFFFFFLL) return fail(MVQ_EINVAL, "%s: n_new = %d", who, n_new);
    const long long q0 = consumed / orig;
    const long long done = q0 > hold ? q0 - hold : 0;                    // blocks emitted by earlier calls
    long long n_out;
    if (final) {
        n_out = ((long long)newf * (consumed + n_new) + orig - 1) / orig - (long long)newf * done;
    } else {
        const long long q1 = q0 + n_new / orig - hold;
        n_out = q1 > done ? (long long)newf * (q1 - done) : 0;
    }
    if (n_out != len_out) return fail(MVQ_EINVAL, "%s: len_out = %d, this call completes %lld outputs", who, len_out, n_out);
    const int base = (int)(q0 < hold ? (hold - q0) * orig : 0);
    const int lead = (int)(consumed < ns ? ns - consumed : 0);
    *p = {(int)ns, (int)n_out, base, lead};
    return MVQ_OK;
}

// The four entry points of the rational streamed resampler: the one-block form and the split form, dense
// and slots, are one argument check and one launcher signature.
using RationalLaunch = hipError_t (*)(const float*, const float*, float*, const int32_t*, float*, int, int, int, int, int, int, int, int, int,
                                      int, hipStream_t);
static int resample_rational_dense(const char* who, RationalLaunch launch, const float* x_new, const float* kern, float* state, float* y,
                                   int batch, int n_new, long long consumed, int final, int len_out, int orig, int newf, int width, int ks,
                                   int hold, void* stream)
{
    ResampleStreamPlan p;
    if (int rc = resample_rational_plan(who, batch, n_new, consumed, final, len_out, orig, newf, width, ks, hold, &p)) return rc;
    if (batch == 0) return MVQ_OK;
    if (!kern || !state || (!x_new && n_new) || (!y && p.n_out)) return fail(MVQ_EINVAL, "%s: null tensor", who);
    hipError_t e = launch(x_new, kern, state, nullptr, y, batch, n_new, p.n_out, orig, newf, ks, p.ns, p.base, p.lead, 0, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, who);
}

static int resample_rational_slots(const char* who, RationalLaunch launch, const float* x_new, const float* kern, float* state,
                                   const int32_t* slots, int n_group, int n_slots, float* y, int n_new, long long consumed, int final,
                                   int len_out, int orig, int newf, int width, int ks, int hold, void* stream)
{
    if (int rc = slots_shape_bad(who, n_group, n_slots, 1)) return rc;
    ResampleStreamPlan p;
    if (int rc = resample_rational_plan(who, n_group, n_new, consumed, final, len_out, orig, newf, width, ks, hold, &p)) return rc;
    if (consumed && consumed < p.ns)
        return fail(MVQ_EINVAL, "%s: consumed = %lld inside the %d-sample state names no launch class (0, or at least %d)", who, consumed,
                    p.ns, p.ns);
    if ((long long)n_group * p.n_out > 0x7FFFFFFFLL) return fail(MVQ_EINVAL, "%s: %d x %d outputs", who, n_group, p.n_out);
    if (n_group == 0) return MVQ_OK;
    if (!kern || !state || !slots || (!x_new && n_new) || (!y && p.n_out)) return fail(MVQ_EINVAL, "%s: null tensor", who);
    hipError_t e = launch(x_new, kern, state, slots, y, n_group, n_new, p.n_out, orig, newf, ks, p.ns, p.base, p.lead, n_slots, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, who);
}

int mvq_resample_stream_rational_f32(const float* x_new, const float* kern, float* state, float* y, int batch, int n_new,
                                     long long consumed, int final, int len_out, int orig, int newf, int width, int ks, int hold,
                                     void* stream)
{
    return resample_rational_dense("resample_stream_rational", mvq::launch_resample_stream_rational, x_new, kern, state, y, batch, n_new,
                                   consumed, final, len_out, orig, newf, width, ks, hold, stream);
}

int mvq_resample_stream_rational_slots_f32(const float* x_new, const float* kern, float* state, const int32_t* slots, int n_group,
                                           int n_slots, float* y, int n_new, long long consumed, int final, int len_out, int orig,
                                           int newf, int width, int ks, int hold, void* stream)
{
    return resample_rational_slots("resample_stream_rational_slots", mvq::launch_resample_stream_rational, x_new, kern, state, slots, n_group,
                                   n_slots, y, n_new, consumed, final, len_out, orig, newf, width, ks, hold, stream);
}

int mvq_resample_stream_rational_split_f32(const float* x_new, const float* kern, float* state, float* y, int batch, int n_new,
                                           long long consumed, int final, int len_out, int orig, int newf, int width, int ks, int hold,
                                           void* stream)
{
    return resample_rational_dense("resample_stream_rational_split", mvq::launch_resample_stream_rational_split, x_new, kern, state, y, batch,
                                   n_new, consumed, final, len_out, orig, newf, width, ks, hold, stream);
}

int mvq_resample_stream_rational_split_slots_f32(const float* x_new, const float* kern, float* state, const int32_t* slots, int n_group,
                                                 int n_slots, float* y, int n_new, long long consumed, int final, int len_out, int orig,
                                                 int newf, int width, int ks, int hold, void* stream)
{
    return resample_rational_slots("resample_stream_rational_split_slots", mvq::launch_resample_stream_rational_split, x_new, kern, state,
                                   slots, n_group, n_slots, y, n_new, consumed, final, len_out, orig, newf, width, ks, hold, stream);
}

// The size checks of the history window, `who` the entry point's name; `sessions` = batch or n_group.
static int stream_window_sizes_bad(const char* who, int sessions, int h_in, int n, int h_out, int cap, int c)
{
    if (h_in < 0 || n < 0 || h_out < 0 || cap < 0 || sessions < 0 || c < 0) return fail(MVQ_EINVAL, "%s: negative size", who);
    if (h_in > cap || h_out > cap) return fail(MVQ_EINVAL, "%s: h_in = %d / h_out = %d exceed the history capacity %d", who, h_in, h_out, cap);
    if ((long long)h_out > (long long)h_in + n) return fail(MVQ_EINVAL, "%s: h_out = %d exceeds h_in + n = %d + %d", who, h_out, h_in, n);
    if ((long long)h_in + n > (1 << 20)) return fail(MVQ_EINVAL, "%s: window of %lld columns", who, (long long)h_in + n);
    return MVQ_OK;
}

int mvq_stream_window_f32(float* hist, int h_in, const float* z_new, int n, float* win, int h_out, int cap, int batch, int c,
                          void* stream)
{
    if (int rc = stream_window_sizes_bad("stream_window", batch, h_in, n, h_out, cap, c)) return rc;
    const size_t rows = (size_t)batch * c;
    if (rows == 0 || h_in + n == 0) return MVQ_OK;
    if (!win || (!hist && (h_in || h_out)) || (!z_new && n)) return fail(MVQ_EINVAL, "stream_window: null tensor");
    if (rows > (size_t)0x7FFFFFFF * 32) return fail(MVQ_EINVAL, "stream_window: too many rows");
    hipError_t e = mvq::launch_stream_window(hist, nullptr, z_new, win, h_in, n, h_out, cap, c, 0, rows, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_window");
}

int mvq_stream_window_slots_f32(float* hist, const int32_t* slots, int n_group, int n_slots, int h_in, const float* z_new, int n,
                                float* win, int h_out, int cap, int c, void* stream)
{
    if (int rc = stream_window_sizes_bad("stream_window_slots", n_group, h_in, n, h_out, cap, c)) return rc;
    if (int rc = slots_shape_bad("stream_window_slots", n_group, n_slots, c)) return rc;
    const size_t rows = (size_t)n_group * c;
    if (rows == 0 || h_in + n == 0) return MVQ_OK;
    if (!slots || !win || (!hist && (h_in || h_out)) || (!z_new && n)) return fail(MVQ_EINVAL, "stream_window_slots: null tensor");
    hipError_t e = mvq::launch_stream_window(hist, slots, z_new, win, h_in, n, h_out, cap, c, n_slots, rows, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_window_slots");
}

// The checks the two stage-window entry points share (`sessions` = batch or n_group); `rows` = sessions * c.
static int stream_stage_window_bad(const char* who, int sessions, size_t tail_stride, int h_in, int src_t, int src_seg, int src_off, int n,
                                   int win_t, int win_seg, int h_out, int cap, int c)
{
    if (int rc = stream_window_sizes_bad(who, sessions, h_in, n, h_out, cap, c)) return rc;
    if (src_t < 0 || src_off < 0 || win_t < 0) return fail(MVQ_EINVAL, "%s: negative size", who);
    if (src_seg < 1 || win_seg < 1 || src_seg > 64 || win_seg > 64) return fail(MVQ_EINVAL, "%s: src_seg = %d / win_seg = %d segments per row", who, src_seg, win_seg);
    if ((long long)src_off + n > src_t) return fail(MVQ_EINVAL, "%s: columns [%d, %d + %d) lie outside the source rows of %d", who, src_off, src_off, n, src_t);
    if (win_t < h_in + n || win_t > (1 << 20)) return fail(MVQ_EINVAL, "%s: window rows of %d columns for h_in + n = %d + %d", who, win_t, h_in, n);
    if ((h_in || h_out) && tail_stride < (size_t)c * cap)
        return fail(MVQ_EINVAL, "%s: a session stride of %zu floats holds no [%d, %d] tail", who, tail_stride, c, cap);
    return MVQ_OK;
}

int mvq_stream_stage_window_f32(float* tail, size_t tail_stride, int h_in, const float* src, int src_t, int src_seg, int src_off, int n,
                                float* win, int win_t, int win_seg, int h_out, int cap, int batch, int c, void* stream)
{
    if (int rc = stream_stage_window_bad("stream_stage_window", batch, tail_stride, h_in, src_t, src_seg, src_off, n, win_t, win_seg, h_out, cap, c))
        return rc;
    const size_t rows = (size_t)batch * c;
    if (rows == 0 || h_in + n == 0) return MVQ_OK;
    if (rows > 0x7FFFFFFFu) return fail(MVQ_EINVAL, "stream_stage_window: too many rows");
    if (!win || (!tail && (h_in || h_out)) || (!src && n)) return fail(MVQ_EINVAL, "stream_stage_window: null tensor");
    hipError_t e = mvq::launch_stream_stage_window(tail, tail_stride, nullptr, src, src_t, src_seg, src_off, win, win_t, win_seg, h_in, n, h_out,
                                                   cap, c, 0, rows, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_stage_window");
}

int mvq_stream_stage_window_slots_f32(float* tail, size_t tail_stride, const int32_t* slots, int n_group, int n_slots, int h_in,
                                      const float* src, int src_t, int src_seg, int src_off, int n, float* win, int win_t, int win_seg,
                                      int h_out, int cap, int c, void* stream)
{
    if (int rc = stream_stage_window_bad("stream_stage_window_slots", n_group, tail_stride, h_in, src_t, src_seg, src_off, n, win_t, win_seg, h_out,
                                         cap, c))
        return rc;
    if (int rc = slots_shape_bad("stream_stage_window_slots", n_group, n_slots, c)) return rc;
    const size_t rows = (size_t)n_group * c;
    if (rows == 0 || h_in + n == 0) return MVQ_OK;
    if (!slots || !win || (!tail && (h_in || h_out)) || (!src && n)) return fail(MVQ_EINVAL, "stream_stage_window_slots: null tensor");
    hipError_t e = mvq::launch_stream_stage_window(tail, tail_stride, slots, src, src_t, src_seg, src_off, win, win_t, win_seg, h_in, n, h_out,
                                                   cap, c, n_slots, rows, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_stage_window_slots");
}

// The stage window with its Snake beside it (the stateful encoder's wide blocks): dense rows only, the same checks.
int mvq_stream_stage_window_snake_f32(float* tail, size_t tail_stride, int h_in, const float* src, int src_t, int src_off, int n, float* win,
                                      float* win_s, const float* alpha, int win_t, int h_out, int cap, int batch, int c, void* stream)
{
    if (int rc = stream_stage_window_bad("stream_stage_window_snake", batch, tail_stride, h_in, src_t, 1, src_off, n, win_t, 1, h_out, cap, c)) return rc;
    const size_t rows = (size_t)batch * c;
    if (rows == 0 || h_in + n == 0) return MVQ_OK;
    if (rows > 0x7FFFFFFFu) return fail(MVQ_EINVAL, "stream_stage_window_snake: too many rows");
    if (!win || !win_s || !alpha || (!tail && (h_in || h_out)) || (!src && n)) return fail(MVQ_EINVAL, "stream_stage_window_snake: null tensor");
    hipError_t e = mvq::launch_stream_stage_window_snake(tail, tail_stride, nullptr, src, src_t, src_off, win, win_s, alpha, win_t, h_in, n, h_out,
                                                         cap, c, 0, rows, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_stage_window_snake");
}

int mvq_stream_stage_window_snake_slots_f32(float* tail, size_t tail_stride, const int32_t* slots, int n_group, int n_slots, int h_in,
                                            const float* src, int src_t, int src_off, int n, float* win, float* win_s, const float* alpha,
                                            int win_t, int h_out, int cap, int c, void* stream)
{
    if (int rc = stream_stage_window_bad("stream_stage_window_snake_slots", n_group, tail_stride, h_in, src_t, 1, src_off, n, win_t, 1, h_out, cap, c))
        return rc;
    if (int rc = slots_shape_bad("stream_stage_window_snake_slots", n_group, n_slots, c)) return rc;
    const size_t rows = (size_t)n_group * c;
    if (rows == 0 || h_in + n == 0) return MVQ_OK;
    if (!slots || !win || !win_s || !alpha || (!tail && (h_in || h_out)) || (!src && n))
        return fail(MVQ_EINVAL, "stream_stage_window_snake_slots: null tensor");
    hipError_t e = mvq::launch_stream_stage_window_snake(tail, tail_stride, slots, src, src_t, src_off, win, win_s, alpha, win_t, h_in, n, h_out,
                                                         cap, c, n_slots, rows, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_stage_window_snake_slots");
}

int mvq_stream_samples_f32(float* buf, int fill, const float* x_new, int n, float* win, int w, int drop, int cap, int rows,
                           void* stream)
{
    if (fill < 0 || n < 0 || w < 0 || drop < 0 || cap < 0 || rows < 0) return fail(MVQ_EINVAL, "stream_samples: negative size");
    if (cap > (1 << 24) || n > (1 << 24)) return fail(MVQ_EINVAL, "stream_samples: cap = %d / n = %d samples per row", cap, n);
    if (fill > cap) return fail(MVQ_EINVAL, "stream_samples: fill = %d exceeds the capacity %d", fill, cap);
    const long long have = (long long)fill + n;
    if (w > have) return fail(MVQ_EINVAL, "stream_samples: w = %d exceeds fill + n = %d + %d", w, fill, n);
    if (drop > have) return fail(MVQ_EINVAL, "stream_samples: drop = %d exceeds fill + n = %d + %d", drop, fill, n);
    if (have - drop > cap) return fail(MVQ_EINVAL, "stream_samples: %lld samples to keep exceed the capacity %d", have - drop, cap);
    if (rows == 0 || (n == 0 && w == 0 && drop == 0)) return MVQ_OK;
    if (!buf || (!x_new && n) || (!win && w)) return fail(MVQ_EINVAL, "stream_samples: null tensor");
    hipError_t e = mvq::launch_stream_samples(buf, nullptr, x_new, win, fill, n, w, drop, cap, rows, 0, 0, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_samples");
}

int mvq_stream_samples_slots_f32(float* buf, const int32_t* desc, int n_group, int n_slots, const float* x_new, int x_total, float* win,
                                 int w, int cap, void* stream)
{
    if (x_total < 0 || w < 0 || cap < 0) return fail(MVQ_EINVAL, "stream_samples_slots: negative size");
    if (int rc = slots_shape_bad("stream_samples_slots", n_group, n_slots, 2)) return rc;
    if (cap > (1 << 24) || w > (1 << 25)) return fail(MVQ_EINVAL, "stream_samples_slots: cap = %d / w = %d samples per row", cap, w);
    if (n_group == 0) return MVQ_OK;
    if (!buf || !desc || (!x_new && x_total) || (!win && w)) return fail(MVQ_EINVAL, "stream_samples_slots: null tensor");
    hipError_t e = mvq::launch_stream_samples(buf, desc, x_new, win, 0, 0, w, 0, cap, n_group, n_slots, x_total, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_samples_slots");
}

int mvq_stream_rows_f32(float* pool, const int32_t* slots, int n_group, int n_slots, float* rows, int c, int scatter, void* stream)
{
    if (c < 0) return fail(MVQ_EINVAL, "stream_rows: negative size");
    if (int rc = slots_shape_bad("stream_rows", n_group, n_slots, c)) return rc;
    if (n_group == 0 || c == 0) return MVQ_OK;
    if (!pool || !slots || !rows) return fail(MVQ_EINVAL, "stream_rows: null tensor");
    hipError_t e = mvq::launch_stream_rows(pool, slots, rows, n_group, c, n_slots, scatter != 0, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "stream_rows");
}

int mvq_hold_fill_slots_f32(float* x, const uint8_t* valid, float* carry_pool, const int32_t* slots, int n_group, int n_slots, int c,
                            int t, void* stream)
{
    if (c < 0 || t < 0 || (c + 15) / 16 > 65535) return fail(MVQ_EINVAL, "hold_fill_slots: bad shape");
    if (int rc = slots_shape_bad("hold_fill_slots", n_group, n_slots, c)) return rc;
    if ((size_t)n_group * c * t == 0) return MVQ_OK;
    if (!x || !valid || !carry_pool || !slots) return fail(MVQ_EINVAL, "hold_fill_slots: null tensor");
    hipError_t e = mvq::launch_hold_fill_slots(x, valid, carry_pool, slots, n_group, n_slots, c, t, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "hold_fill_slots");
}

// The one argument check of the audio fade (`who`: the entry point; `sessions` = batch or n_group) -> the launch's `back` (the piece
// starts that many tokens in front of the step's new ones) and `fresh` (nothing came before the step).  The step's tokens fix len:
// a push emits 320*(n - 10 + back) samples, a finish 320*(n + back) - 8.
struct AudioFadePlan { int back, fresh; };
static int audio_fade_plan(const char* who, int sessions, int n, int tok0, int len, int hold_tok, int fade_tok, AudioFadePlan* p)
{
    if (sessions < 0 || n < 0 || tok0 < 0 || len < 0) return fail(MVQ_EINVAL, "%s: negative size", who);
    if (hold_tok < 0 || fade_tok < 1 || (long long)hold_tok + fade_tok > 255)
        return fail(MVQ_EINVAL, "%s: hold_tok = %d, fade_tok = %d (hold_tok >= 0, fade_tok >= 1, hold_tok + fade_tok <= 255)", who, hold_tok, fade_tok);
    if (n > (1 << 22) || len > (1 << 30)) return fail(MVQ_EINVAL, "%s: n = %d tokens / len = %d samples", who, n, len);
    long long back;
    if (len % 320 == 320 - 8) back = (long long)(len + 8) / 320 - n;                     // a finish: up to the item's last sample
    else if (len % 320 == 0) back = (long long)len / 320 + 10 - n;                       // a push: up to 10 tokens behind the newest
    else return fail(MVQ_EINVAL, "%s: len = %d is no 320*m (a push) and no 320*m - 8 (a finish)", who, len);
    if (back < 0 || back > 10 || (tok0 > 0 && back != 10))
        return fail(MVQ_EINVAL, "%s: a piece of %d samples from token %d on is not what a step of %d new tokens emits", who, len, tok0, n);
    p->back = (int)back;
    p->fresh = tok0 == 0 && back == 0;
    return MVQ_OK;
}

int mvq_audio_fade_f32(float* y, const uint8_t* valid, int32_t* state, int batch, int n, int tok0, int len, int hold_tok, int fade_tok,
                       void* stream)
{
    AudioFadePlan p;
    if (int rc = audio_fade_plan("audio_fade", batch, n, tok0, len, hold_tok, fade_tok, &p)) return rc;
    if (batch == 0) return MVQ_OK;
    if (!state || (!y && len) || (!valid && n)) return fail(MVQ_EINVAL, "audio_fade: null tensor");
    hipError_t e = mvq::launch_audio_fade(y, valid, state, nullptr, batch, 0, len, n, p.back, p.fresh, hold_tok, fade_tok, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "audio_fade");
}

int mvq_audio_fade_slots_f32(float* y, const uint8_t* valid, int32_t* state, const int32_t* slots, int n_group, int n_slots, int n,
                             int tok0, int len, int hold_tok, int fade_tok, void* stream)
{
    AudioFadePlan p;
    if (int rc = audio_fade_plan("audio_fade_slots", n_group, n, tok0, len, hold_tok, fade_tok, &p)) return rc;
    if (int rc = slots_shape_bad("audio_fade_slots", n_group, n_slots, 1)) return rc;
    if (n_group == 0) return MVQ_OK;
    if (!state || !slots || (!y && len) || (!valid && n)) return fail(MVQ_EINVAL, "audio_fade_slots: null tensor");
    hipError_t e = mvq::launch_audio_fade(y, valid, state, slots, n_group, n_slots, len, n, p.back, p.fresh, hold_tok, fade_tok, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "audio_fade_slots");
}

int mvq_sumsq_partial_f32(const float* x, float* partial, int n_partial, size_t n, void* stream)
{
    if (!partial || n_partial <= 0 || n_partial > 4096 || (!x && n)) return fail(MVQ_EINVAL, "sumsq_partial: bad argument");
    hipError_t e = mvq::launch_sumsq_partial(x, partial, n_partial, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "sumsq_partial");
}

int mvq_adamw_f32(float* p, const float* g, float* m, float* v, const float* clip_coef, size_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, void* stream)
{
    if (step < 1 || beta1 < 0 || beta1 >= 1 || beta2 < 0 || beta2 >= 1) return fail(MVQ_EINVAL, "adamw: bad hyper-parameter");
    if ((!p || !g || !m || !v) && n) return fail(MVQ_EINVAL, "adamw: null tensor");
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    hipError_t e = mvq::launch_adamw(p, g, m, v, clip_coef, n, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)sqrt(bc2), S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "adamw");
}

int mvq_mul_dtanh_f32(const float* g, const float* y, float* out, size_t n, void* stream)
{
    if ((!g || !y || !out) && n) return fail(MVQ_EINVAL, "mul_dtanh: null tensor");
    hipError_t e = mvq::launch_mul_dtanh(g, y, out, n, S(stream));
    return e == hipSuccess ? MVQ_OK : hipfail(e, "mul_dtanh");
}

}  // extern "C"
