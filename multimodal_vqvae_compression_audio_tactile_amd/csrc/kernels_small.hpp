// kernels_small.hpp -- launchers of the non-GEMM kernels (kernels_small.hip, kernels_vq.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace mvq {

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, DEVICE): one flag per device ordinal, so a process that
// drives several GPUs opts every one of them in (a single per-process flag would leave the second device at the 64 KB default).
constexpr int kMaxLdsOptInDevices = 64;
struct BigLdsOptIn {
    bool done[kMaxLdsOptInDevices] = {};
    hipError_t ensure(const void* kern)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const bool tracked = dev >= 0 && dev < kMaxLdsOptInDevices;
        if (tracked && done[dev]) return hipSuccess;
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
        if (e == hipSuccess && tracked) done[dev] = true;
        return e;
    }
};

int prof_begin(const char* kernel_name, double flops, hipStream_t s);     // api.hip (see conv1d_mfma.hpp)
void prof_end(int idx, hipStream_t s);
bool prof_enabled();

struct DirectConvArgs {
    const float* x; const float* wp; const float* bias; const float* alpha_in; const float* residual;
    const float* alpha_out; float* y;
    int B, Cin, Tin, Cout, Tout, ks, stride, dil, pad, Mpad, act;
    float* y2; const float* alpha2;       // dual output (see ConvArgs::y2)
    const float* dsn_src; const float* dsn_alpha;   // dgrad epilogue (see ConvArgs::dsn_src)
};

hipError_t launch_weight_norm(const float* v, const float* g, float* w, int rows, int inner, hipStream_t s);
hipError_t launch_pack_conv1d(const float* w, float* wp, int cin, int cout, int ks, int mpad, hipStream_t s);
hipError_t launch_pack_convtr(const float* w, float* wp, int cin, int cout, int S, int mpad, hipStream_t s);
hipError_t launch_conv1d_direct(const DirectConvArgs& a, hipStream_t s);
hipError_t launch_convtr_direct(const DirectConvArgs& a, hipStream_t s);
hipError_t launch_layernorm_c(const float* x, const float* pe, const float* gamma, const float* beta, float* y,
                              int B, int C, int T, size_t sb, size_t sc, float eps, int do_tanh, float post_scale,
                              const float* sub, hipStream_t s);
// Which kernel launch_layernorm_c runs for n = B * T tokens of C channels: decided here and nowhere else (host arithmetic, no device).
enum class LnForm { Lat, Tile8, Tile4, Scalar };
LnForm layernorm_form(int n, int C);
const char* layernorm_form_name(LnForm f);                    // the instantiation as rocprofv3 prints it
hipError_t launch_attention(const float* q, const float* k, const float* v, float* ctx,
                            int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                            hipStream_t s);
hipError_t launch_attention_masked(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                                   int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                                   size_t msb, hipStream_t s);
hipError_t launch_hold_fill(float* x, const uint8_t* valid, float* carry, int B, int C, int T, hipStream_t s);
hipError_t launch_hold_fill_slots(float* x, const uint8_t* valid, float* carry_pool, const int32_t* slots, int G, int n_slots, int C,
                                  int T, hipStream_t s);
hipError_t launch_gelu(const float* x, float* y, size_t n, hipStream_t s);
hipError_t launch_strided3d(const float* a, size_t asb, size_t asc, const float* b2, size_t bsb, size_t bsc,
                            float* y, size_t ysb, size_t ysc, int B, int C, int n, hipStream_t s);

hipError_t launch_pack_conv1d_dgrad(const float* w, float* wp, int cin, int cout, int ks, int mpad, hipStream_t s);
hipError_t launch_pack_convtr_dgrad(const float* w, float* wp, int cin, int cout, int ks, int mpad, hipStream_t s);
hipError_t launch_mul_dtanh(const float* g, const float* y, float* out, size_t n, hipStream_t s);
hipError_t launch_layernorm_bwd(const float* x, const float* pe, const float* gamma, const float* g, float* gx,
                                float* dgamma, float* dbeta, float* stats, int B, int C, int T, size_t sb, size_t sc,
                                float eps, hipStream_t s);
hipError_t launch_gelu_bwd(const float* x, const float* g, float* gx, size_t n, hipStream_t s);
hipError_t launch_scale_tanh(const float* u, float s, float* y, size_t n, hipStream_t st);
hipError_t launch_scale_tanh_bwd(const float* u, const float* g, float s, float* gu, float* partial, int n_partial, size_t n,
                                 hipStream_t st);
hipError_t launch_attention_bwd(const float* q, const float* k, const float* v, const float* g, float* gq, float* gk, float* gv,
                                int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc, hipStream_t s);
hipError_t launch_attention_masked_bwd(const float* q, const float* k, const float* v, const uint8_t* kmask, const float* g,
                                       float* gq, float* gk, float* gv, int B, int H, int dh, int Tq, int Tk,
                                       size_t qsb, size_t qsc, size_t ksb, size_t ksc, size_t msb, hipStream_t s);
bool attn_seq_plan(int dh, int tk, int* qt, int* kt, size_t* lds_floats);      // attention_seq.hip
hipError_t launch_attention_seq(const float* q, const float* k, const float* v, float* ctx,
                                int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc, hipStream_t s);
hipError_t launch_attention_seq_masked(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                                       int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb, size_t ksc,
                                       size_t msb, hipStream_t s);
hipError_t launch_attention_seq_bwd(const float* q, const float* k, const float* v, const float* g, float* gq, float* gk, float* gv,
                                    float* scratch, int B, int H, int dh, int Tq, int Tk, size_t qsb, size_t qsc, size_t ksb,
                                    size_t ksc, hipStream_t s);
hipError_t launch_attention_seq_masked_bwd(const float* q, const float* k, const float* v, const uint8_t* kmask, const float* g,
                                           float* gq, float* gk, float* gv, float* scratch, int B, int H, int dh, int Tq, int Tk,
                                           size_t qsb, size_t qsc, size_t ksb, size_t ksc, size_t msb, hipStream_t s);
hipError_t launch_channel_draw(uint8_t* out, int B, int T, int ptok, int nb, int min_books, uint64_t thr_loss, uint64_t thr_thin,
                               uint64_t thr_gb, uint64_t thr_bg, uint64_t thr_loss_bad, uint32_t h_stream, uint32_t item_base,
                               hipStream_t s);                                                             // channel.hip
hipError_t launch_plc_mask_fill(const float* zt, const float* zp, const uint8_t* mask, float* zt_in, float* zf,
                                int B, int C, int T, size_t sb, size_t sc, hipStream_t s);
hipError_t launch_plc_mask_fill_bwd(const float* g, const uint8_t* mask, float* gzp, int B, int C, int T, size_t sb, size_t sc,
                                    hipStream_t s);
hipError_t launch_frame_subsets(const uint8_t* lat, int t_lat, double spt, int hop, int t_f, uint8_t* fmask, int* cols_m,
                                int* cols_u, int* counts, hipStream_t s);                                  // mel_ssim.hip
hipError_t launch_mel_ssim(const float* M, size_t ld, const float* maxv, int n_maxv, const int* desc, const int* cols, size_t n_cols,
                           const int* widths, int n, int max_width, int mode, double* out, hipStream_t s);
hipError_t launch_subset_stats(const float* ref, const float* est, int T, const uint8_t* lat, int t_lat, float spt, double* out,
                               hipStream_t s);
hipError_t launch_mul_scaled(const float* a, const float* b, float scale, float* out, size_t n, hipStream_t s);
hipError_t launch_transpose2d(const float* in, float* out, int rows, int cols, hipStream_t s);
hipError_t launch_rowsum(const float* in, float* out, int rows, int cols, int accumulate, hipStream_t s);
hipError_t launch_stft_frames(const float* x, const float* window, float* out, int B, int T, int n_fft, int hop, int nframes,
                              size_t ncols, size_t col0, hipStream_t s);
hipError_t launch_spec_mag(const float* S, float* mag, int F, int Fp, size_t ncols, float eps, hipStream_t s);
hipError_t launch_spec_loss_partial(const float* mag, float* partial, int P, int F, int B, int nframes, size_t ncols, hipStream_t s);
hipError_t launch_spec_grad(const float* S, const float* mag, const float* coefA, float coefB, const float* extra, float* G,
                            int F, int Fp, int B, int nframes, size_t ncols, float eps, hipStream_t s);
hipError_t launch_overlap_add(const float* dF, const float* window, float* dy, int B, int T, int n_fft, int hop, int nframes, hipStream_t s);
hipError_t launch_l1_loss(const float* y, const float* tgt, float* partial, int P, float* dy, float coef, size_t n, hipStream_t s);
hipError_t launch_mel_max(const float* M, float* maxv, int* argm, int n_mels, int B, int nframes, size_t ncols, hipStream_t s);
hipError_t launch_mel_cos(const float* M, const float* maxv, float* cosv, float* dM, float* dden, float coef, int n_mels, int B,
                          int nframes, size_t ncols, float eps, int use_log, hipStream_t s);
hipError_t launch_mel_max_grad(const float* dden, const float* maxv, const int* argm, float* dM, int B, int nframes, float eps, hipStream_t s);
hipError_t launch_resample(const float* x, const float* kern, float* y, int B, int L, int Lout, int orig, int newf,
                           int width, int ks, hipStream_t s);
hipError_t launch_sumsq_partial(const float* x, float* partial, int n_partial, size_t n, hipStream_t s);
hipError_t launch_adamw(float* p, const float* g, float* m, float* v, const float* clip_coef, size_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, float bc1, float sqrt_bc2, hipStream_t s);
hipError_t launch_align_xcorr_batch(const float* r, const float* e, int B, int T, int max_shift, float* corr, int* scratch_valid,
                                    int* best_shift, hipStream_t s);
hipError_t launch_resample_ragged(const float* x, const float* kern, float* y, const int* off, const int* len, int* lout, int B,
                                  int pitch, int lout_pitch, int orig, int newf, int width, int ks, hipStream_t s);
hipError_t launch_align_xcorr(const float* r, const float* e, int T, int max_shift, float* corr, int* scratch_valid,
                              int* best_shift, hipStream_t s);

hipError_t launch_rvq_ema_forward(const float* z, const float* books, float* q_out, int32_t* idx_out,
                                  int B, int D, int T, int nb, int K, int update_residual, hipStream_t s);
// Which kernel launch_rvq_ema_forward runs for N = B * T tokens (host arithmetic, no device).  tpb: live tokens per block of the
// MFMA form (16 or 32), 0 for every other form.
enum class RvqForm { Rows, Token, Tile8, Mfma, Tile32 };
struct RvqChoice { RvqForm form; int tpb; };
RvqChoice rvq_ema_forward_form(int N, int D, int K, bool books_aligned);
void rvq_ema_forward_form_name(RvqChoice c, char* buf, int len);
// ... and launch_dac_rvq (C in {256, 512, 1024}; `prepared`: both prepared tensors given; `aligned`: in_w, out_w, codebook and
// the prepared codebook all 16-byte aligned).  Invalid: a width no kernel is compiled for.
enum class DacRvqForm { Lat1, Lat2, Tile, Invalid };
DacRvqForm dac_rvq_form(int N, int C, int K, bool prepared, bool aligned);
void dac_rvq_form_name(DacRvqForm f, int C, char* buf, int len);
size_t ema_update_scratch_bytes(int N, int nb, int K, int D);
hipError_t launch_ema_update(const float* z, const int32_t* idx, float* books, void* scratch, int B, int D, int T, int nb, int K,
                             float decay, hipStream_t s);
hipError_t launch_dac_rvq(const float* z, const float* in_w, const float* in_b, const float* cb, const float* out_w,
                          const float* out_b, float* zq, int32_t* codes, float* latents, const int32_t* nq_item,
                          int B, int C, int T, int nq, int K, int Dc, hipStream_t s,
                          const float* cbn_pre = nullptr, const float* cn2_pre = nullptr);
hipError_t launch_dac_rvq_prepare(const float* cb, float* cbn, float* cn2, int nq, int K, int Dc, hipStream_t s);
hipError_t launch_rvq_dequant(const int64_t* idx, const float* books, float* q, int B, int D, int T, int nb, int K,
                              size_t out_sb, size_t out_sd, hipStream_t s);
hipError_t launch_dac_rvq_from_codes(const int64_t* codes, const float* cb, const float* out_w, const float* out_b, float* zq,
                                     float* z_p, int B, int C, int T, int nq, int K, int Dc, hipStream_t s);
hipError_t launch_dac_rvq_from_codes_layers(const int64_t* codes, size_t codes_sb, const float* cb, const float* out_w, const float* out_b,
                                            const uint8_t* nq_valid, float* zq, float* z_p, int B, int C, int T, int nq, int K, int Dc,
                                            hipStream_t s);
// packets.hip: the lossy-channel receiver (bits = ceil(log2 K) <= 24, ptok >= 1)
hipError_t launch_idx_pack_packets(const int64_t* idx, uint8_t* bodies, int B, int nb, int T, int K, int bits, int ptok,
                                   size_t s_book, size_t s_item, hipStream_t s);
hipError_t launch_idx_unpack_packets(const uint8_t* bodies, const uint8_t* nb_recv, int64_t* idx, uint8_t* nb_valid, int B, int nb,
                                     int T, int K, int bits, int ptok, hipStream_t s);
hipError_t launch_rvq_dequant_layers(const int64_t* idx, const float* books, const uint8_t* nb_valid, float* q, int B, int D, int T,
                                     int nb, int K, size_t out_sb, size_t out_sd, hipStream_t s);
// fec.hip: r parity rows per group over GF(2^8) (1 <= r <= 4; r = 1 is XOR parity) over the first m books of groups of g packets
// (1 <= g <= 16, 1 <= m <= nb; B * ceil(P / g) <= INT_MAX): rows[B, G, r, g + W]; the parities of a group that arrived are the bits
// of got & got_mask, at r = 1 "any bit"
hipError_t launch_fec_parity(const uint8_t* bodies, const uint8_t* nb_sent, uint8_t* rows, int B, int nb, int T, int bits, int ptok,
                             int g, int m, int r, hipStream_t s);
hipError_t launch_fec_recover(uint8_t* bodies, uint8_t* nb_recv, const uint8_t* rows, const uint8_t* got, uint8_t* recovered, int B,
                              int nb, int T, int bits, int ptok, int g, int m, int r, uint32_t got_mask, hipStream_t s);
// rate.hip: closed-loop sender rate control (mvq_rvq_rate_f32); rvq_rate_check returns an MVQ_* code, its text through set_last_error
int rvq_rate_check(int dim, int nb_use, int k, int packet_tok, int group_tok, int min_books, int mode, float tol2, int budget,
                   const char* who = "rvq_rate");     // ``who`` prefixes the message (the audio rate control passes its own name)
hipError_t launch_rvq_rate(const float* z, size_t z_sb, size_t z_sd, const int32_t* idx, size_t idx_sbook, size_t idx_sitem,
                           const float* books, float* q_out, size_t out_sb, size_t out_sd, uint8_t* nb_valid, size_t nbv_sb,
                           uint8_t* nb_sent, size_t nbs_sb, float* energy, int B, int D, int T, int nb, int K, int ptok, int gtok,
                           int min_books, int mode, float tol2, int budget, hipStream_t s);
// rvq_beam.hip: beam search over the books at the sender (mvq_rvq_beam_f32); rvq_beam_check returns an MVQ_* code, its text through
// set_last_error; both strided like launch_rvq_rate's z and idx, slot / energy (either may be nullptr) contiguous [B*T]
int rvq_beam_check(int dim, int nb_use, int k, int beam, const char* who = "rvq_beam");
hipError_t launch_rvq_beam(const float* z, size_t z_sb, size_t z_sd, const float* books, int32_t* idx, size_t idx_sbook, size_t idx_sitem,
                           uint8_t* slot, float* energy, int B, int D, int T, int nb, int K, int beam, hipStream_t s);
// stream.hip: the streaming receiver's state kernels (rows = batch*c; S = ceil(width/orig)*orig + width <= 1024).  slots ==
// nullptr: every session of the buffers, densely; else the G sessions slots[G] (a device list) of a pool of n_slots, C rows per
// session and rows = G*C <= INT_MAX
hipError_t launch_stream_stage_window(float* tail, size_t tail_stride, const int32_t* slots, const float* src, int src_t, int src_seg,
                                      int src_off, float* win, int win_t, int win_seg, int h_in, int n, int h_out, int cap, int C,
                                      int n_slots, size_t rows, hipStream_t s);
hipError_t launch_stream_stage_window_snake(float* tail, size_t tail_stride, const int32_t* slots, const float* src, int src_t, int src_off,
                                            float* win, float* win_s, const float* alpha, int win_t, int h_in, int n, int h_out, int cap,
                                            int C, int n_slots, size_t rows, hipStream_t s);
hipError_t launch_stream_window(float* hist, const int32_t* slots, const float* z_new, float* win, int h_in, int n, int h_out, int cap,
                                int C, int n_slots, size_t rows, hipStream_t s);
hipError_t launch_resample_stream(const float* x_new, const float* kern, float* state, const int32_t* slots, float* y, int B, int n_new,
                                  int n_out, int orig, int ks, int S, int base, int lead, int n_slots, hipStream_t s);
hipError_t launch_resample_stream_rational(const float* x_new, const float* kern, float* state, const int32_t* slots, float* y, int B,
                                           int n_new, int n_out, int orig, int newf, int ks, int S, int base, int lead, int n_slots,
                                           hipStream_t s);
// the split form: an outputs launch over (parts, sessions), then the state launch (one block per session)
hipError_t launch_resample_stream_rational_split(const float* x_new, const float* kern, float* state, const int32_t* slots, float* y, int B,
                                                 int n_new, int n_out, int orig, int newf, int ks, int S, int base, int lead, int n_slots,
                                                 hipStream_t s);
hipError_t launch_stream_rows(float* pool, const int32_t* slots, float* rows, int G, int C, int n_slots, int scatter, hipStream_t s);
// stream.hip: the receiver's audio output, the fade of lost tokens (one block per session; state[sessions][11] int32)
hipError_t launch_audio_fade(float* y, const uint8_t* valid, int32_t* state, const int32_t* slots, int G, int n_slots, int len, int n,
                             int back, int fresh, int H, int F, hipStream_t s);
// stream.hip: the streaming sender's sample state (one block per row of buf[rows][cap])
hipError_t launch_stream_samples(float* buf, const int32_t* desc, const float* x_new, float* win, int fill, int n, int w, int drop,
                                 int cap, int rows, int n_slots, int x_total, hipStream_t s);
}  // namespace mvq
