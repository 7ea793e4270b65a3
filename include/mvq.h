/*
 * mvq.h -- C ABI of libmvq_hip.so: the MI355X (gfx950) encode -> vector-quantise -> decode hot path of
 * aymenboudhina/Multimodal_VQVAE_compression_audio_tactile.
 *
 * The reference has no FFI: its boundary is the Python object surface its scripts touch
 * (SURVEY.md section 8b).  Each entry point below names the reference call it replaces
 * (paths relative to /root/reference).  All pointers are DEVICE pointers (HIP), all tensors fp32,
 * contiguous, channel-major [B, C, T] exactly as torch lays them out, indices int32 on this ABI
 * (the Python mirror widens to int64).  `stream` is a hipStream_t passed as void* (NULL = default
 * stream).  Inputs are borrowed and never written; outputs must be caller-allocated.
 * Every function returns 0 on success or a negative MVQ_E* code; mvq_last_error() gives the text.
 * No function allocates, frees or synchronises (safe to capture into a hipGraph), except
 * mvq_device_query() and the mvq_profile_* pair.
 *
 * Arithmetic contract: every dot product is one fp32 fma chain in the order "input channel ascending,
 * then tap ascending" starting from +0.0f, followed by  + bias, + residual, snake, tanh  (each optional).
 * On gfx950 that is what a k-ordered v_mfma_f32_32x32x2_f32 accumulation yields, so results are
 * bit-reproducible and comparable bit for bit with oracle/c/oracle.c.
 */
#ifndef MVQ_H
#define MVQ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVQ_OK 0
#define MVQ_EINVAL (-1)      /* bad shape / argument                     */
#define MVQ_EUNSUPPORTED (-2)/* shape outside what the kernels cover     */
#define MVQ_EHIP (-3)        /* HIP runtime error (launch failure, ...)  */

#define MVQ_ACT_NONE 0
#define MVQ_ACT_TANH 1
#define MVQ_ACT_GELU 2   /* exact-erf GELU (nn.GELU() of CrossPredictor.ffn); MFMA-tiled, non-transposed shapes only */

/* ABI version.  3 (round 5): whole-stack entry points (additive since, same version: the full-sequence attention pair
 * mvq_attention_seq_f32 / mvq_attention_seq_bwd_f32 with mvq_attention_seq_bwd_scratch_bytes, and mvq_plc_mask_fill_f32 /
 * mvq_plc_mask_fill_bwd_f32 of the packet-loss-concealment model, and its evaluation: mvq_frame_subsets, mvq_mel_ssim_f32,
 * mvq_subset_stats_f32; the lossy-channel receiver: mvq_idx_pack_packets_u8, mvq_idx_unpack_packets, mvq_rvq_dequant_layers_f32;
 * forward error correction: mvq_fec_parity_u8, mvq_fec_recover_u8, mvq_fec_rs_parity_u8, mvq_fec_rs_recover_u8; audio concealment: mvq_attention_masked_f32,
 * mvq_attention_seq_masked_f32, mvq_hold_fill_f32; the audio/FEC pools: mvq_hold_fill_slots_f32; training under the link:
 * mvq_attention_masked_bwd_f32, mvq_attention_seq_masked_bwd_f32, mvq_channel_draw_u8;
 * the streaming receiver: mvq_stream_window_f32, mvq_resample_stream_f32; the streaming sender: mvq_stream_samples_f32,
 * mvq_ar_latents_staged_carry_f32; the receiver pool: mvq_stream_window_slots_f32, mvq_resample_stream_slots_f32,
 * mvq_stream_rows_f32; the sender pool: mvq_stream_samples_slots_f32; sender rate control: mvq_rvq_rate_f32,
 * mvq_ar_latents_staged_rate_f32; the sender's beam search: mvq_rvq_beam_f32, mvq_ar_latents_staged_rate_beam_f32; audio transport: mvq_dac_rvq_from_codes_layers_f32, mvq_dac_rvq_rate_f32,
 * mvq_dac_rvq_rate_workspace_bytes; the stateful streaming decoder: mvq_stream_stage_window_f32, mvq_stream_stage_window_slots_f32,
 * mvq_decoder_stream_plan, mvq_decoder_stream_state_floats, mvq_decoder_stream_workspace_bytes, mvq_decoder_stream_fwd_f32; the
 * stateful streaming encoder: mvq_stream_stage_window_snake_f32, mvq_stream_stage_window_snake_slots_f32, mvq_encoder_stream_plan,
 * mvq_encoder_stream_state_floats, mvq_encoder_stream_workspace_bytes, mvq_encoder_stream_fwd_f32; the receiver's audio output:
 * mvq_audio_fade_f32, mvq_audio_fade_slots_f32; the native-rate sender: mvq_resample_stream_rational_f32,
 * mvq_resample_stream_rational_slots_f32; their split form for few sessions: mvq_resample_stream_rational_split_f32,
 * mvq_resample_stream_rational_split_slots_f32; fine-tuning the decoder: mvq_conv1d_wgrad_workspace_bytes, mvq_conv1d_wgrad_f32,
 * mvq_channel_reduce_workspace_bytes, mvq_snake_bwd_f32, mvq_bias_grad_f32, mvq_weight_norm_bwd_f32).
 * Whole-stack entry points (mvq_encoder_fwd_f32, mvq_decoder_fwd_f32, mvq_decoder_fwd_saving_f32,
 * mvq_decoder_bwd_input_f32 and the mvq_stack handle).  2 (round 4): mvq_rvq_ema_step_f32 takes the larger 16-byte-aligned scratch that
 * mvq_rvq_ema_step_scratch_bytes() reports (version 1 documented nb*B*T int32), mvq_profile_end2() reports truncation,
 * mvq_build_flags() exists. */
int mvq_abi_version(void);
const char* mvq_last_error(void);
/* How this library is being driven: 0 when no A/B override is in the environment.
 *   0x100 MVQ_NO_DMA is set: the conv K loops stage through registers instead of LDS-DMA (results stay correct, timings are not
 *   the product's).  All other bits are reserved and never set.
 * The Python mirror refuses to load a library whose low 16 bits are non-zero unless MVQ_ALLOW_TIMING_BUILD=1;
 * bench.py prints the value in its line. */
unsigned mvq_build_flags(void);

/* Per-launch HIP-event profiler (measurement aid of bench.py; no reference counterpart).  Between mvq_profile_begin() and
 * mvq_profile_end() every conv / residual-unit kernel launch of the library is bracketed by a HIP event pair recorded on
 * the stream it is launched on, together with the launch's ALGORITHMIC FLOPs (2 * Cin * ks * valid rows * valid columns *
 * batch: zero-padded rows and tail tiles are not counted).  mvq_profile_end() waits for the events (it synchronises) and
 * returns one entry per kernel instantiation -- the name is the one rocprofv3 prints -- with the summed duration, FLOPs and
 * launch count.  Not capturable into a hipGraph while enabled; one profiling session per process at a time (global state,
 * not thread-safe). */
typedef struct mvq_profile_entry {
    char kernel[96];
    double seconds;
    double flops;
    int launches;
} mvq_profile_entry;
int mvq_profile_begin(void);
/* writes at most max_entries rows; *n_entries = the number of rows WRITTEN (instantiations beyond the buffer are dropped).
 * Returns MVQ_EHIP when an event could not be created or recorded during the session (first such error; nothing is written). */
int mvq_profile_end(mvq_profile_entry* out, int max_entries, int* n_entries);
/* same, and *n_total = the number of instantiations the session recorded: *n_total > *n_entries means the table was truncated */
int mvq_profile_end2(mvq_profile_entry* out, int max_entries, int* n_entries, int* n_total);
/* creates the event pairs of n_launches launches ahead of time: call it before a timed region so that no hipEventCreate
 * falls inside it (events are pooled and reused across sessions). */
int mvq_profile_reserve(int n_launches);
/* fills cu_count / lds_bytes / gcn arch name ("gfx950...") of the current device; synchronous. */
int mvq_device_query(int* cu_count, int* lds_bytes_per_cu, char* arch, int arch_len);

/* ---- one-off weight preparation (model load time) -------------------------------------------- */

/* torch.nn.utils.weight_norm fold, dim 0:  w[r,:] = v[r,:] * (g[r] / ||v[r,:]||_2).
 * Replaces the implicit fold inside every upstream dac WNConv1d / WNConvTranspose1d forward that
 * dac.DAC.load(...) modules perform (Training/compare_dacvsproposal_5.py:329-338). */
int mvq_weight_norm_f32(const float* v, const float* g, float* w, int rows, int inner, void* stream);

/* Packed (K-major, zero-padded) weight image used by mvq_conv1d_f32:  wp[(ci*ks + kk) * Mpad + co].
 * Query the size (in floats) first, then pack from the torch layout w[Cout, Cin, ks]. */
size_t mvq_conv1d_packed_floats(int cin, int cout, int ks);
int mvq_conv1d_pack_f32(const float* w, float* wp, int cin, int cout, int ks, void* stream);

/* Same for ConvTranspose1d with kernel = 2*stride (every upstream DecoderBlock): torch layout
 * w[Cin, Cout, 2*stride] -> polyphase image wp[(ci*2 + j) * Mpad + (co*stride + r)]. */
size_t mvq_conv_transpose1d_packed_floats(int cin, int cout, int stride);
int mvq_conv_transpose1d_pack_f32(const float* w, float* wp, int cin, int cout, int stride, void* stream);

/* ---- conv stack primitives ---------------------------------------------------------------------- */

/* y = act( snake_out( conv1d( snake_in(x) ) + bias + residual ) ).
 * Replaces torch F.conv1d + the surrounding Snake1d / residual add / tanh inside dac Encoder / Decoder /
 * ResidualUnit, the 1x1 proj_down / proj_up convs (Training/compare_dacvsproposal_5.py:287-288) and the
 * bias-free nn.Linear layers of CrossPredictor (...:226-228) when applied on channel-major tensors.
 *   x[B,Cin,Tin], wp from mvq_conv1d_pack_f32, bias[Cout]|NULL, alpha_in[Cin]|NULL (Snake1d before
 *   the conv), residual[B,Cout,Tout]|NULL, alpha_out[Cout]|NULL (Snake1d after), act MVQ_ACT_*.
 *   Tout = (Tin + 2*pad - dil*(ks-1) - 1)/stride + 1.   y[B,Cout,Tout]. */
int mvq_conv1d_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                   const float* residual, const float* alpha_out, float* y,
                   int batch, int cin, int tin, int cout, int ks, int stride, int dil, int pad, int act,
                   void* stream);

/* Dual-output forms.  Besides y they write  y2 = snake(v, alpha2)  where v is the value before alpha_out / act
 * (conv + bias + residual): the Snake1d that the NEXT ResidualUnit applies to its input, hoisted into the producer so
 * that a consumer with M/128 row tiles does not re-evaluate it M/128 times per element while staging.  y2[B,Cout,Tout],
 * alpha2[Cout]; pass both or neither (NULL, NULL == the plain entry points above / below). */
int mvq_conv1d_dual_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                        const float* residual, const float* alpha_out, float* y, float* y2, const float* alpha2,
                        int batch, int cin, int tin, int cout, int ks, int stride, int dil, int pad, int act,
                        void* stream);
int mvq_conv_transpose1d_dual_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                  const float* alpha_out, float* y, float* y2, const float* alpha2,
                                  int batch, int cin, int tin, int cout, int stride, int pad, void* stream);

/* Name of the kernel instantiation the two conv entry points launch for a shape ("conv1d_mfma_kernel<...>" as
 * rocprofv3 prints it, or "conv1d_direct_kernel"): lets bench.py match its HIP-event timings to the trace.  Tile shape
 * depends on batch and length (64 x 64 tiles in the latency regime, 128 x 96 at the latent rate); "same"/DAC padding is
 * assumed.  For transposed convs pass the torch shape (cin, cout, ks = 2*stride, stride). */
int mvq_conv_kernel_name(int batch, int cin, int cout, int ks, int stride, int dil, int transposed, int tin,
                         char* buf, int len);
/* The same for the three forward entry points that choose a kernel by token count (batch * t), width and alignment:
 * mvq_layernorm_c_f32 / _sub_f32, mvq_rvq_ema_forward_f32 (and the assignment pass of mvq_rvq_ema_step_f32) and
 * mvq_dac_rvq_*_f32.  Host arithmetic: nothing is launched and no device is needed; batch, t >= 1.
 *   layernorm:  "layernorm_c_lat_kernel" | "layernorm_c_tile_kernel<8>" | "layernorm_c_tile_kernel<4>" | "layernorm_c_kernel"
 *   rvq search: "rvq_ema_forward_rows_kernel<24>" | "rvq_ema_forward_token_kernel" | "rvq_ema_forward_kernel<8>" | "<32>" |
 *               "rvq_ema_forward_mfma_kernel [tpb=16]" | "[tpb=32]" (one kernel; live tokens per block are an argument).
 *               books_aligned: the books pointer is 16-byte aligned.
 *   dac rvq:    "dac_rvq_lat_kernel<C/16, 4, 1>" | "<C/16, 4, 2>" | "dac_rvq_kernel<C/16, 8>".  prepared: cb_normalised and
 *               cb_norm2 are given; aligned: in_w, out_w, codebook and cb_normalised are all 16-byte aligned. */
int mvq_layernorm_kernel_name(int batch, int c, int t, char* buf, int len);
int mvq_rvq_ema_forward_kernel_name(int batch, int dim, int t, int k, int books_aligned, char* buf, int len);
int mvq_dac_rvq_kernel_name(int batch, int c, int t, int k, int prepared, int aligned, char* buf, int len);

/* One upstream dac ResidualUnit:  y = snake_next?( x + conv1( snake_b( conv7_dil( snake_a(x) ) + b7 ) ) + b1 ),
 * 7-tap conv with dilation `dil` and padding 3*dil, then a 1x1 conv, both C -> C.  For C in {64, 96, 128} (the
 * high-rate ends of the stacks, where the 1x1 conv is bandwidth-bound on its own) the whole unit is ONE launch and
 * the intermediate never leaves the CU; otherwise two launches through `scratch` (B*C*T floats, see
 * mvq_residual_unit_scratch_floats; may be NULL when that returns 0).  alpha_next: the following Snake1d or NULL. */
size_t mvq_residual_unit_scratch_floats(int batch, int c, int t, int dil);
int mvq_residual_unit_kernel_name(int c, int dil, char* buf, int len);   /* "residual_unit_kernel<...>" or "(two launches)" */
int mvq_residual_unit_f32(const float* x, const float* w7p, const float* b7, const float* alpha_a,
                          const float* alpha_b, const float* w1p, const float* b1, const float* alpha_next,
                          float* y, float* scratch, int batch, int c, int t, int dil, void* stream);

/* ResidualUnit with a pre-snaked input and/or dual output: x_snaked = snake_a(x) (from a producer's y2) or NULL;
 * y2 = snake(y_raw, alpha2) for the next unit or NULL. */
int mvq_residual_unit_dual_f32(const float* x, const float* x_snaked, const float* w7p, const float* b7,
                               const float* alpha_a, const float* alpha_b, const float* w1p, const float* b1,
                               const float* alpha_next, float* y, float* y2, const float* alpha2, float* scratch,
                               int batch, int c, int t, int dil, void* stream);

/* y = snake_out( conv_transpose1d( snake_in(x) ) + bias ), kernel = 2*stride, torch `padding` = pad.
 * Replaces the Snake1d + WNConvTranspose1d at the head of every upstream DecoderBlock.
 *   Tout = (Tin-1)*stride - 2*pad + 2*stride. */
int mvq_conv_transpose1d_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                             const float* alpha_out, float* y,
                             int batch, int cin, int tin, int cout, int stride, int pad, void* stream);

/* ---- vector quantisation ------------------------------------------------------------------------ */

/* ResidualVQEMA.forward (Training/compare_dacvsproposal_5.py:256-265; eval variant with n_books_use
 * Evaluation/dac_vcpwq_proposed6_latency.py:417-435).  z[B,D,T], books[nb_use,K,D] contiguous.
 * Per token and book: idx = argmax_k(res.e_k - 0.5*||e_k||^2) (lowest index on ties), q = e[idx],
 * q_sum = (q_sum + (q - res)) + res, res = res - q.   q_out[B,D,T]; idx_out[nb_use, B*T] may be NULL. */
int mvq_rvq_ema_forward_f32(const float* z, const float* books, float* q_out, int32_t* idx_out,
                            int batch, int dim, int t, int nb_use, int k, void* stream);

/* ResidualVQEMA.ema_step (Training/compare_dacvsproposal_5.py:266-277): every book matched against the
 * SAME tokens X = z_tokens[B,D,T]; used codes move to decay*e + (1-decay)*mean(assigned tokens).
 * books[nb,K,D] updated in place.  scratch: mvq_rvq_ema_step_scratch_bytes() bytes, 16-byte aligned (the per-book
 * assignments nb*B*T int32, then the workspace of a stable counting sort of the token ids by code + the token-major copy
 * of X).  Per (code, dim) the sum runs over the code's OWN tokens in token order -- the additions index_add_ performs, in
 * its order, so the result is deterministic and bit-equal to the sequential loop -- at O(B*T*D) work per book instead of
 * O(K*D*B*T).  B*T < 2^24 (counts stay exact in fp32), K <= 16384. */
size_t mvq_rvq_ema_step_scratch_bytes(int batch, int t, int nb, int k, int dim);
int mvq_rvq_ema_step_f32(const float* z_tokens, float* books, void* scratch,
                         int batch, int dim, int t, int nb, int k, float decay, void* stream);

/* dac ResidualVectorQuantize.forward in eval mode, first nq_use stages
 * (`qa, *_ = self.A_QUANT(za)` Training/compare_dacvsproposal_5.py:295; `mdl.encode(x, n_quantizers)`
 * Evaluation/compare_dacvsproposal_5_eval.py:369).  Weights already weight-norm folded:
 *   in_w[nq,Dc,C], in_b[nq,Dc], codebook[nq,K,Dc], out_w[nq,C,Dc], out_b[nq,C].
 *   z[B,C,T] -> zq[B,C,T], codes[B,nq_use,T] (int32), latents[B,nq_use*Dc,T].   C in {256, 512, 1024}, Dc = 8.
 * Summation order of in_proj (the only C-long reduction here): 16 block partials over C/16 contiguous channels
 * (each an fma chain from +0), added in block order, then + bias; out_proj: fma chain over Dc, then + bias. */
int mvq_dac_rvq_f32(const float* z, const float* in_w, const float* in_b, const float* codebook,
                    const float* out_w, const float* out_b, float* zq, int32_t* codes, float* latents,
                    int batch, int c, int t, int nq_use, int k, int dc, void* stream);
/* The same with upstream's TRAIN-mode quantiser dropout (dac ResidualVectorQuantize.forward under `net.train()`,
 * Training/compare_dacvsproposal_5.py:401): every stage runs, item b's zq sums only stages < nq_item[b]
 * (nq_item[batch] int32 on the device, NULL = no dropout); codes / latents of all nq_use stages are produced. */
int mvq_dac_rvq_items_f32(const float* z, const float* in_w, const float* in_b, const float* codebook,
                          const float* out_w, const float* out_b, float* zq, int32_t* codes, float* latents,
                          const int32_t* nq_item, int batch, int c, int t, int nq_use, int k, int dc, void* stream);
/* One-off preparation of the quantiser's codebooks (model load time, like the weight-norm fold): cb_normalised[nq,K,Dc] =
 * F.normalize(codebook) and cb_norm2[nq,K] = its squared norms, by the same divisions / fma chains the search kernel would
 * otherwise redo in every block of every call (a fifth of its vector instructions).  mvq_dac_rvq_prepared_f32 is
 * mvq_dac_rvq_items_f32 with those two tensors handed in (both NULL = normalise in the kernel): bit-identical outputs. */
int mvq_dac_rvq_prepare_f32(const float* codebook, float* cb_normalised, float* cb_norm2, int nq, int k, int dc, void* stream);
int mvq_dac_rvq_prepared_f32(const float* z, const float* in_w, const float* in_b, const float* codebook,
                             const float* cb_normalised, const float* cb_norm2,
                             const float* out_w, const float* out_b, float* zq, int32_t* codes, float* latents,
                             const int32_t* nq_item, int batch, int c, int t, int nq_use, int k, int dc, void* stream);


/* The receiver's look-ups (what the transmitted indices decode to; the straight-through forms of the two quantisers above cannot
 * be reproduced without the encoder-side residual).  Every index read is clamped to [0, K), so a corrupt index cannot read out
 * of bounds; indices are int64 as the Python side holds them.
 * ResidualVQEMA dequantise: idx[nb_use, B*T] (token b*T+t), books[>=nb_use, K, D] (16-byte aligned, D % 4 == 0):
 *   q(b,d,t) = ((+0 + e_0[idx_0][d]) + e_1[idx_1][d]) + ...  in book order (nb_use = 0 writes zeros),
 *   stored at b*out_sb + d*out_sd + t: [B,D,T] is (D*T, T) (0,0 = that), the token-folded [D, B*T] is (T, B*T). */
int mvq_rvq_dequant_f32(const int64_t* idx, const float* books, float* q_out, int batch, int dim, int t, int nb_use, int k,
                        size_t out_sb, size_t out_sd, void* stream);
/* dac ResidualVectorQuantize.from_codes: codes[B,nq_use,T]; codebook[>=nq_use,K,Dc], out_w[.,C,Dc], out_b[.,C] as in
 * mvq_dac_rvq_f32 (codebook and out_w 16-byte aligned).  p_i = codebook_i[code_i] (the raw row); zq_i(c) = fma chain over the
 * Dc code dims ascending from +0, then + out_b; zq = ((0 + zq_0) + zq_1) + ... in stage order -> zq[B,C,T];
 * z_p[B,nq_use*Dc,T] = the raw rows (NULL = not written).  C % 64 == 0, nq_use <= 32, Dc = 8. */
int mvq_dac_rvq_from_codes_f32(const int64_t* codes, const float* codebook, const float* out_w, const float* out_b, float* zq,
                               float* z_p, int batch, int c, int t, int nq_use, int k, int dc, void* stream);

/* The lossy-channel receiver (additive, same ABI version; no reference counterpart: the reference's PLC model masks the encoder's
 * own latents).  A tactile item of T tokens travels as P = ceil(T / packet_tok) packets; packet p carries tokens
 * [p*packet_tok, min(T, (p+1)*packet_tok)), ntok of them.  Its body holds nb*ntok indices of bits = ceil(log2 K) bits each,
 * BOOK-major (element e = book*ntok + j at bits [e*bits, (e+1)*bits)), each index least-significant bit first, bits packed
 * LSB-first into bytes; body_full = ceil(nb*packet_tok*bits / 8) bytes, a row is zero past its last element (pad bits, and the
 * shorter tail packet).  packets.py (pack_bodies / unpack_bodies) is the numpy definition these kernels equal bit for bit.
 * Covered: nb <= 255, 1 <= packet_tok <= 255, bits <= 24; anything else is MVQ_EINVAL "bad shape" before any launch.
 *
 * Pack: index (book i, item b, token t) is read at idx[i*s_book + b*s_item + t] (idx[nb,B,T]: (B*T, T); codes[B,nq,T]: (T, nq*T)),
 * clamped to [0, K).  Writes EVERY byte of bodies[B, P, body_full].  One thread owns one byte: no atomics. */
int mvq_idx_pack_packets_u8(const int64_t* idx, uint8_t* bodies, int batch, int nb, int t, int k, int packet_tok,
                            size_t s_book, size_t s_item, void* stream);
/* Unpack: bodies[B, P, body_full] and nb_recv[B, P] (books of the packet that arrived; 0 = lost; values above nb count as nb)
 * -> idx[nb, B*T] (token b*T+t, the layout mvq_rvq_dequant_f32 reads) and nb_valid[B*T] = the token's packet's count.  Books at or
 * above the count are written as 0; a value >= K is clamped to K-1, so a corrupt body cannot make a later look-up read out of
 * bounds.  Writes every element of both outputs. */
int mvq_idx_unpack_packets(const uint8_t* bodies, const uint8_t* nb_recv, int64_t* idx, uint8_t* nb_valid, int batch, int nb, int t,
                           int k, int packet_tok, void* stream);
/* mvq_rvq_dequant_f32 with a per-token book count nb_valid[B*T] (token b*T+t; NULL = mvq_rvq_dequant_f32 itself):
 *   q(b,d,t) = ((+0 + e_0[idx_0][d]) + e_1[idx_1][d]) + ...  over the first min(nb_use, nb_valid[b*T+t]) books; a count of 0
 * writes +0 (RVQ is successively refinable: a partly delivered token is a lower-rate token).  Same strided output. */
int mvq_rvq_dequant_layers_f32(const int64_t* idx, const float* books, const uint8_t* nb_valid, float* q_out, int batch, int dim,
                               int t, int nb_use, int k, size_t out_sb, size_t out_sd, void* stream);

/* Closed-loop sender rate control (additive, same ABI version; no reference counterpart).  After the search of a chunk the SENDER
 * decides how many books each packet carries and forms, from exactly those books, the sum the receiver will form
 * (mvq_rvq_dequant_layers_f32's arithmetic), so that the AR history of both ends is the same bits at any rate.
 * Per item the t tokens fall into groups of group_tok (the AR chunk, 16; the last may be shorter) and packets of packet_tok
 * (packet_tok divides group_tok).  Per token, with r_0 = z(b, :, t) and the indices the search returned:
 *   r_{m+1}[d] = r_m[d] - e_m[idx_m][d];   E_m = (...((+0 + r_m[0]*r_m[0]) + r_m[1]*r_m[1]) + ...), d ascending, the multiply and
 *   the add rounded separately (no fma), m = 0 .. nb_use.
 * MVQ_RATE_FULL: every packet carries nb_use books.  MVQ_RATE_TOL2 (constant quality): need(token) = the smallest m in
 * [min_books, nb_use] with E_m <= tol2 * E_0 (one fp32 multiply; nb_use when there is none: a NaN compares false), a packet
 * carries the max over its tokens.  MVQ_RATE_BUDGET (constant rate): the packets of a group share `budget` books
 * (a group of g < P_c = group_tok / packet_tok packets: max(g*min_books, budget*g / P_c)); every packet starts at min_books, then
 * book by book the packet with the largest gain = (...(+0 + (E_m[j] - E_{m+1}[j])) + ...) over its tokens j gets its next one --
 * candidates (packets below nb_use) in ascending order, the first is the incumbent, a later one replaces it only when its gain
 * compares strictly greater -- until the budget is spent or every packet has nb_use.
 * z (b, d, t) is read at b*z_sb + d*z_sd + t, index (book i, item b, token t) at idx[i*idx_sbook + b*idx_sitem + t] (int32 as the
 * search writes it, clamped to [0, K)); a stride pair of 0 means contiguous.  Writes EVERY element of q_out (strided like
 * mvq_rvq_dequant_f32's: the sum over the first nb_valid books), nb_valid[b*nbv_sb + t] (the count of the token's packet),
 * nb_sent[b*nbs_sb + p] (packet p of the item; P = ceil(t / packet_tok)) and, unless NULL, energy[nb_use + 1, batch*t].
 * nb_use == 0 writes zeros and counts of 0.  Covered: D % 4 == 0, D <= 128, nb_use <= 32, group_tok <= 16 (else MVQ_EUNSUPPORTED);
 * 1 <= min_books <= nb_use, a finite tol2 > 0, P_c*min_books <= budget <= P_c*nb_use, packet_tok | group_tok (else MVQ_EINVAL):
 * all before any launch.  One block per (item, group); no atomics. */
#define MVQ_RATE_FULL 0
#define MVQ_RATE_TOL2 1
#define MVQ_RATE_BUDGET 2
int mvq_rvq_rate_f32(const float* z, size_t z_sb, size_t z_sd, const int32_t* idx, size_t idx_sbook, size_t idx_sitem,
                     const float* books, float* q_out, size_t out_sb, size_t out_sd, uint8_t* nb_valid, size_t nbv_sb,
                     uint8_t* nb_sent, size_t nbs_sb, float* energy, int batch, int dim, int t, int nb_use, int k,
                     int packet_tok, int group_tok, int min_books, int mode, float tol2, int budget, void* stream);

/* Beam search over the books at the sender (additive, same ABI version; no reference counterpart).  The
 * search above is greedy: book by book argmax_k(res.e_k - 0.5|e_k|^2).  This one keeps up to M = beam slots per token and returns the
 * path with the smallest FINAL residual energy; it costs no bit on the wire and nothing at the receiver, which sums whatever
 * indices arrive.  Every step is one IEEE fp32 operation.  Per token, r = z(b, :, t):
 *   score(r, m, k) = dot - h_k, the greedy search's own value: dot = the fma(r[d], e_m[k][d], dot) chain, d ascending from +0,
 *                    h_k = 0.5 * (the fma(e[d], e[d], s) chain, d ascending from +0);
 *   E(r)           = mvq_rvq_rate_f32's energy chain (...((+0 + r[0]*r[0]) + r[1]*r[1]) + ...), multiply and add rounded separately.
 * A token carries L <= M slots (path, residual r_j, J_j = E(r_j)); before book 0, L = 1 and slot 0 is (empty, r, E(r)).  At book m:
 *   slot 0, the greedy lineage: k* = argmax_k score(r_0, m, k), strict '>' in ascending k (lowest index on ties; no score that
 *     compares greater than -inf -- an all-NaN row -- gives 0); new slot 0 = path_0 + k*;
 *   the other slots, from all pairs (j < L, k < K) except (0, k*): key(j, k) = fl(J_j - fl(2 * score(r_j, m, k))); new slots
 *     1 .. min(M, L*K) - 1 are the pairs first in the order: a number before a NaN, then key ascending (-0 == +0), then j ascending,
 *     then k ascending;
 *   every new slot: r' = r_parent - e_m[k] elementwise (the search's res - q), J' = E(r'); L <- min(M, L*K).
 * After the last book the winner is the slot with the smallest J, strict '<' in ascending slot order (ties and NaN stay with slot
 * 0); the output is its path.  So beam = 1 is the greedy search index for index, and for every token the winner's final energy is
 * <= the greedy path's as an exact fp32 comparison.  The beam optimises the full depth nb_use: a PREFIX of its path (what a thinned
 * packet or a tol2 / budget cut sends) is not the greedy prefix and may be worse; mvq_rvq_rate_f32 decides on the path's own E_m.
 * z and idx are strided as mvq_rvq_rate_f32's (z (b, d, t) at b*z_sb + d*z_sd + t; index (book i, item b, token t) at
 * idx[i*idx_sbook + b*idx_sitem + t]; a stride pair of 0 means contiguous [B, D, T] / [nb_use, B*T]).  Writes EVERY element of idx
 * (int32) and, unless NULL, slot[batch*t] (uint8: the winning slot, 0 = the greedy path won) and energy[batch*t] (the winner's J).
 * Refused before any launch (MVQ_EINVAL): beam outside 1..8, D % 4 != 0 or D > 128, K <= 0 (or above 2^24), nb_use > 32, a null
 * z / idx / books, books not 16-byte aligned.  One block per 1 - 8 tokens for all books; no atomics. */
int mvq_rvq_beam_f32(const float* z, size_t z_sb, size_t z_sd, const float* books, int32_t* idx, size_t idx_sbook, size_t idx_sitem,
                     uint8_t* slot, float* energy, int batch, int dim, int t, int nb_use, int k, int beam, void* stream);

/* Forward error correction (additive, same ABI version; no reference counterpart, and the format is not derived from anything the
 * reference contains).  Bodies are book-major, so the first m books of a body are a valid lower-rate body: one XOR parity row over
 * the first m = books books of every group = g consecutive packets is unequal error protection whose repaired packet is a packet
 * thinned to m books -- mvq_idx_unpack_packets and the layered look-ups treat it as any lower-rate token.  Parity group j of an item
 * covers packets [j*g, min(P, (j+1)*g)), G = ceil(P / g) groups; packet p is protected to c_p = min(m, nb_sent[p]) books;
 * prefix(p) = the first ceil(c_p*ntok_p*bits / 8) bytes of body row p, the bits of book c_p and above cleared in the last one,
 * zero-extended to W = ceil(m*packet_tok*bits / 8).  Row j of rows[B, G, g + W]: bytes 0..g-1 = c_p of the group's packets (0 in the
 * slots of a short tail group), bytes g..g+W-1 = the XOR of the group's prefixes.  packets.py (fec_rows / fec_recover) is the numpy
 * definition these kernels equal bit for bit.  Refused before any launch (MVQ_EINVAL "bad shape"): group outside 1..16, books
 * outside 1..nb, and the shapes mvq_idx_pack_packets_u8 refuses; batch == 0 or t == 0 is a no-op.
 *
 * Parity: bodies[B, P, body_full], nb_sent[B, P] (NULL = every packet carries nb books) -> rows_out.  One thread owns one output
 * byte and XORs the at most 16 masked body bytes that fall into it; writes EVERY byte of rows_out; no atomics. */
int mvq_fec_parity_u8(const uint8_t* bodies, const uint8_t* nb_sent, uint8_t* rows_out, int batch, int nb, int t, int k, int packet_tok,
                      int group, int books, void* stream);
/* Recovery, in place on bodies[B, P, body_full] and nb_recv[B, P] (what mvq_idx_unpack_packets reads), from rows[B, G, g + W] and
 * got[B, G] (0 = the group's parity did not arrive).  For a group with got != 0 and c_p = min(count byte, m, nb) -- clamped, so a
 * corrupt parity packet cannot make a read leave its row -- packet p is deficient when nb_recv[p] < c_p (lost, or thinned below its
 * protected count).  When EXACTLY ONE packet q of the group is deficient: row q = (XOR bytes) ^ XOR_{p != q} prefix(p) over its
 * first ceil(c_q*ntok_q*bits / 8) bytes and zero past them, nb_recv[q] = c_q, recovered[q] = 1.  In every other case the group is
 * left exactly as it arrived.  One block per (item, group); only the deficient row and its count are written, the count behind a
 * barrier after every thread of the block has made its decision; recovered[B, P] (NULL = not written) has every element written.
 * No atomics. */
int mvq_fec_recover_u8(uint8_t* bodies, uint8_t* nb_recv, const uint8_t* rows, const uint8_t* got, uint8_t* recovered, int batch, int nb,
                       int t, int k, int packet_tok, int group, int books, void* stream);

/* Reed-Solomon parity (additive, same ABI version; no reference counterpart): parity = r rows per group, 1 <= r <= 4, a systematic
 * MDS erasure code over GF(2^8) (polynomial x^8+x^4+x^3+x^2+1 = 0x11d, generator 2).  Packet u of its group (u < g <= 16) has the
 * coefficient A[i][u] = 2^(i*u) in parity i; every square submatrix of the 4 x 16 matrix A is nonsingular.  rows[B, G, r, g + W]:
 * row [j, i] = the g count bytes of the XOR row, then the GF sum over the group's packets of A[i][u] * prefix(u), so row [j, 0] IS
 * the XOR row of mvq_fec_parity_u8.  Refused before any launch (MVQ_EINVAL "bad shape"): what the XOR entry points refuse, and
 * parity outside 1..4; batch == 0 or t == 0 is a no-op.  packets.py (fec_rows / fec_recover with Fec.parity) is the numpy
 * definition.  Parity: one thread per output byte, EVERY byte of rows_out written, no atomics. */
int mvq_fec_rs_parity_u8(const uint8_t* bodies, const uint8_t* nb_sent, uint8_t* rows_out, int batch, int nb, int t, int k,
                         int packet_tok, int group, int books, int parity, void* stream);
/* Recovery in place, as mvq_fec_recover_u8, from rows[B, G, r, g + W] and got[B, G], a BITMASK: bit i set = parity i of the group
 * arrived (bits at and above r are ignored).  The counts c_p = min(count byte, m, nb) come from the lowest arrived parity; D = the
 * deficient packets (nb_recv[p] < c_p), ascending.  When 1 <= |D| <= (arrived parities): with i_k the |D| LOWEST arrived indices,
 * per byte the syndromes S_k = parity_{i_k} ^ sum_{u not in D} A[i_k][u] * prefix(u), the system M x = S with M[k][d] = A[i_k][q_d]
 * is solved (Gauss-Jordan without pivoting on the inverse, once per block) and every q in D gets row q = x_q over its first
 * ceil(c_q*ntok_q*bits / 8) bytes and zero past them, nb_recv[q] = c_q, recovered[q] = 1.  In every other case the group is left
 * exactly as it arrived.  One block of 64 threads per (item, group); rows of D are only written, the others only read; the counts
 * are written behind a barrier; recovered[B, P] (NULL = not written) has every element written.  No atomics, no tables.  With
 * parity == 1 and got in {0, 1} both entry points compute what the XOR entry points compute. */
int mvq_fec_rs_recover_u8(uint8_t* bodies, uint8_t* nb_recv, const uint8_t* rows, const uint8_t* got, uint8_t* recovered, int batch,
                          int nb, int t, int k, int packet_tok, int group, int books, int parity, void* stream);

/* Audio transport (additive, same ABI version; no reference counterpart).  The DAC quantiser is a residual VQ, so the first m stages
 * of a token's codes are a valid lower-rate code: the audio codes travel in the layered packets of the tactile stream
 * (mvq_idx_pack_packets_u8 with the codes[B,nq,T] strides) and the receiver sums what arrived.
 *
 * mvq_dac_rvq_from_codes_f32 with a per-token stage count nq_valid[B*T] (uint8, token b*T+t): token (b, t) sums only its first
 * min(nq_use, nq_valid[b*T+t]) stages, in mvq_dac_rvq_from_codes_f32's arithmetic (the same chain cut short); a count of 0 writes
 * +0 for every channel, no bias.  Item b's code rows start at codes + b*codes_sb (0 = nq_use*t, contiguous; larger: the first
 * nq_use rows of a taller tensor, read in place).  z_p (NULL = not written) holds the raw rows of all nq_use stages whatever the
 * count.  nq_valid = NULL with contiguous codes IS mvq_dac_rvq_from_codes_f32 (the same launch); every code read is clamped to
 * [0, K); every element of zq is written.  C % 64 == 0, nq_use <= 32, Dc = 8. */
int mvq_dac_rvq_from_codes_layers_f32(const int64_t* codes, size_t codes_sb, const float* codebook, const float* out_w, const float* out_b,
                                      const uint8_t* nq_valid, float* zq, float* z_p, int batch, int c, int t, int nq_use, int k, int dc,
                                      void* stream);
/* Closed-loop audio rate control: after the DAC quantiser has produced codes[B, >= na_use, T] for z[B,C,T] (the fp32 encoder output it
 * quantised), the SENDER decides how many stages each audio packet carries and forms, from exactly those stages, the qa the receiver
 * will form (mvq_dac_rvq_from_codes_layers_f32 on the counts this call writes).  Per token, with S_0(c) = +0 and
 *   S_{m+1}(c) = S_m(c) + zq_m(c)   (from_codes's own running sum),   d_m(c) = z(c) - S_m(c),   p_m(c) = fl(d_m(c) * d_m(c)),
 *   E_m = sum of p_m over the C channels, m = 0 .. na_use, every multiply and add a separate fp32 operation (no fma), in this
 * FIXED order, a function of the channel alone (not of B, T, the grid or where the token sits):
 *   t(s, g) = (((+0 + p(64s + g)) + p(64s + g + 16)) + p(64s + g + 32)) + p(64s + g + 48)     s = 0 .. C/64 - 1, g = 0 .. 15
 *   P(s)    = (...((+0 + t(s, 0)) + t(s, 1)) + ...) + t(s, 15)
 *   E_m     = (...((+0 + P(0)) + P(1)) + ...) + P(C/64 - 1).
 * The decision is mvq_rvq_rate_f32's rule (one device function serves both), with books = stages, nb_use = na_use, group_tok = 16
 * tokens from token 0 of each item (the last group may be shorter) and the same mode / min_books / tol2 / budget arguments.
 * Writes EVERY element of qa_out[B,C,T], na_valid[B*T] (the count of the token's packet), na_sent[B, P = ceil(t / packet_tok)] and,
 * unless NULL, energy[na_use + 1, B*T].  workspace: mvq_dac_rvq_rate_workspace_bytes(batch, c, t, na_use) bytes of device memory
 * (the per-slab partial energies; written and read by this call only).  Three launches: partial energies over (16 tokens x 64
 * channels) blocks, one block per (item, group) that adds the partials in slab order and decides, then the layered look-up.  No
 * atomics.  Refused before any launch: C % 64 != 0, Dc != 8, na_use outside 1..32 (MVQ_EUNSUPPORTED / MVQ_EINVAL), packet_tok not a
 * divisor of 16 and a rate outside mvq_rvq_rate_f32's ranges (MVQ_EINVAL). */
size_t mvq_dac_rvq_rate_workspace_bytes(int batch, int c, int t, int na_use);
int mvq_dac_rvq_rate_f32(const float* z, const int64_t* codes, size_t codes_sb, const float* codebook, const float* out_w,
                         const float* out_b, float* qa_out, uint8_t* na_valid, uint8_t* na_sent, float* energy, float* workspace,
                         size_t workspace_bytes, int batch, int c, int t, int na_use, int k, int dc, int packet_tok, int min_books,
                         int mode, float tol2, int budget, void* stream);

/* ---- predictor / glue primitives (CrossPredictor, TokenNorm, PosEnc1D) --------------------------- */

/* y = post_scale * tanh?( LayerNorm_C(x + pe?) ), normalising over the channel axis (eps, biased variance).
 * Element (b, c, t) of x and y lives at  b*stride_b + c*stride_c + t ; pass stride_b = stride_c = 0 for a
 * contiguous [B,C,T] tensor.  (The AR loop keeps chunk tensors token-folded as [C, B*Tc]: stride_b = Tc,
 * stride_c = B*Tc, so that the predictor GEMMs see N = B*Tc contiguous columns.)
 * pe[max_len, C] (row = position) or NULL; positions are 0..T-1 (PosEnc1D restarts per call).
 * Replaces PosEnc1D + ln_q/ln_kv/ffn[0] (Training/compare_dacvsproposal_5.py:236-238,243) and
 * torch.tanh(TokenNorm(r)) * scale (...:313-315). */
int mvq_layernorm_c_f32(const float* x, const float* pe, const float* gamma, const float* beta, float* y,
                        int batch, int c, int t, size_t stride_b, size_t stride_c,
                        float eps, int do_tanh, float post_scale, void* stream);
/* The same on x - sub (element-wise, same addressing): the AR residual r = zt - z_pred followed by tanh(TokenNorm(r))*scale
 * (Training/compare_dacvsproposal_5.py:312-315) in one launch; sub may be NULL. */
int mvq_layernorm_c_sub_f32(const float* x, const float* sub, const float* pe, const float* gamma, const float* beta, float* y,
                            int batch, int c, int t, size_t stride_b, size_t stride_c,
                            float eps, int do_tanh, float post_scale, void* stream);

/* softmax(Q K^T / sqrt(dh)) V per head (Training/compare_dacvsproposal_5.py:239-242).  Q, ctx: (b,c,i) at
 * b*q_stride_b + c*q_stride_c + i ; K, V: (b,c,j) at b*k_stride_b + c*k_stride_c + j (0,0 = contiguous).
 * Tk may be 0 (ctx = 0).  Tq, Tk <= 64 and dh*(Tq+2Tk)+Tq*Tk <= 16384 floats (one head slice lives in LDS). */
int mvq_attention_f32(const float* q, const float* k, const float* v, float* ctx,
                      int batch, int heads, int dh, int tq, int tk,
                      size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, void* stream);

/* The same attention for whole sequences: the CrossPredictor of the packet-loss-concealment model runs once over the full
 * latent sequence (PLC/PLC1.py:349-422; Tq = Tk = T_lat, 75 per 1-s segment, up to the PosEnc1D bound of 8192).  Same
 * addressing and the same arithmetic as mvq_attention_f32 (oracle/c/oracle.c::orc_attention order: score = one fma chain
 * over d ascending from +0 divided by sqrtf(dh); max; det_exp; l summed over j ascending; p_j / l; ctx[d] one fma chain
 * over j ascending), so on every shape mvq_attention_f32 accepts the results are bit-equal.  Tq, Tk <= 8192; Tk may be 0
 * (ctx = 0).  Larger shapes, or a dh whose query tile does not fit 160 KiB of LDS, return MVQ_EINVAL before any launch. */
int mvq_attention_seq_f32(const float* q, const float* k, const float* v, float* ctx,
                          int batch, int heads, int dh, int tq, int tk,
                          size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, void* stream);

/* Attention under a KEY MASK (the receiver's audio concealment "mask": a lost audio token is not a key).  kmask is uint8,
 * item b's key j at b*m_stride_b + j, nonzero = present; J(b) = the ascending list of present j.  The result is bit-equal to
 * mvq_attention_f32 / mvq_attention_seq_f32 on the item's K and V with the columns compacted to J(b) and Tk = |J(b)|: in the
 * order of oracle/c/oracle.c::orc_attention, score = one fma chain over d ascending from +0 divided by sqrtf(dh); max, det_exp
 * and l over J ascending; p_j / l; ctx[d] one fma chain over J ascending.  |J(b)| = 0 gives ctx = +0 for that item.  The K and V
 * values of an absent column never reach the result (NaN or 1e30 there changes nothing): the chunk kernel compacts while it
 * stages (one ballot per wave, slot = popcount of the present keys below), the sequence kernel skips absent columns in every
 * pass (their e_j is +0, whose addition to l is exact; the value chain is predicated, not multiplied).  kmask == NULL is the
 * unmasked launch.  Shape limits, addressing and refusals (before any launch) are those of the unmasked entry points.
 * The backward is mvq_attention_masked_bwd_f32 / mvq_attention_seq_masked_bwd_f32 below. */
int mvq_attention_masked_f32(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                             int batch, int heads, int dh, int tq, int tk,
                             size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, size_t m_stride_b,
                             void* stream);
int mvq_attention_seq_masked_f32(const float* q, const float* k, const float* v, const uint8_t* kmask, float* ctx,
                                 int batch, int heads, int dh, int tq, int tk,
                                 size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, size_t m_stride_b,
                                 void* stream);

/* Hold fill (the receiver's audio concealment "hold"), in place on contiguous x[batch, c, t]: y[b,c,t] = x[b,c,s(b,t)] with
 * s(b,t) the largest t' <= t with valid[b,t'] != 0 (valid: uint8 [batch, t]); where there is none, carry[b,c] (carry: [batch, c]
 * or NULL = +0).  Afterwards carry[b,c] = y[b,c,t-1] (t > 0), so a sequence is filled piece by piece.  Pure copies: -0, NaN and
 * inf pass unchanged.  Only tokens with valid == 0 are written. */
int mvq_hold_fill_f32(float* x, const uint8_t* valid, float* carry, int batch, int c, int t, void* stream);
/* The same for the sessions of a pool (the same kernel body under slot addressing): item g of x[n_group, c, t] / valid[n_group, t]
 * reads and writes the carry row slots[g] of carry_pool[n_slots, c]; rows no slot names are untouched.  A slot outside
 * [0, n_slots) has no row: +0 is read as the carry and none is stored (the caller refuses such a list, and a repeated slot, on
 * the host).  carry_pool and slots are required; n_group <= n_slots. */
int mvq_hold_fill_slots_f32(float* x, const uint8_t* valid, float* carry_pool, const int32_t* slots, int n_group, int n_slots,
                            int c, int t, void* stream);

/* Audio fade (the receiver's audio OUTPUT; packets.AudioFade is the definition): the waveform of audio tokens
 * that never arrived fades out and back in.  With v[t] = "some stage of audio token t arrived":
 *   r[-1] = 0;  r[t] = v[t] ? 0 : min(r[t-1] + 1, H + F)                  H = hold_tok >= 0, F = fade_tok >= 1, H + F <= 255
 *   g[-1] = 1;  g[t] = r[t] <= H ? 1.0f : (float)(H + F - r[t]) / (float)F       one IEEE division
 *   sample s = 320*t + j:  gain = g[t-1] + (g[t] - g[t-1]) * ((float)(j + 1) / 320.0f)    each operation rounded, no fma
 *                          y[s] = gain == 0 ? +0 : y[s] * gain
 * so a sample between two gains of 1 keeps its value (-0 and a quiet NaN keep their bits) and a sample of gain 0 is +0 whatever it
 * held -- predicated, not multiplied.  In place on a PIECE y[batch, 1, len] that starts at a token border, sample 320*tok0 of the
 * item, for the step that brings valid[batch, n] (uint8, nonzero = arrived), the counts of its n new tokens.  The piece is what a
 * streaming step emits (stream.schedule): with `back` = the tokens of the piece in front of the new ones, a push has
 * len = 320*(n - 10 + back) -- it ends 10 tokens (DEC_HALO_TOK) behind the newest -- and a finish len = 320*(n + back) - 8; back is
 * thereby a function of n and len, 0 <= back <= 10 and back == 10 unless tok0 == 0.  The whole item is the finish with tok0 = 0,
 * n = T, len = 320*T - 8.
 * state[sessions, 11] int32, updated in place: r of the last DEC_HALO_TOK + 1 = 11 tokens received, the current run last -- the 10
 * tokens not yet emitted and the one in front of them, whose gain the first sample of the next piece starts from.  Zeros mean "no
 * loss so far"; with tok0 == 0 and back == 0 (a session's first step) the row is not read at all, so a new session needs no
 * clearing.  ONE launch, one block per session: the block reads its row, a barrier, then it stores the row; no row and no sample
 * is touched by two blocks.  No host read.
 * MVQ_EINVAL before any launch: fade_tok < 1, hold_tok < 0, hold_tok + fade_tok > 255, a negative size, a len that is not the
 * sample count of such a step, a null pointer where data is needed (state always; y with len > 0; valid with n > 0).  batch = 0
 * returns MVQ_OK without a launch.
 * mvq_audio_fade_slots_f32: the same kernel body for the sessions slots[n_group] of a pool, state[n_slots, 11]; the slot rules of
 * the receiver pool below (a slot outside [0, n_slots) reads "no loss so far" and stores no row; n_group = 0: no launch). */
int mvq_audio_fade_f32(float* y, const uint8_t* valid, int32_t* state, int batch, int n, int tok0, int len, int hold_tok, int fade_tok,
                       void* stream);
int mvq_audio_fade_slots_f32(float* y, const uint8_t* valid, int32_t* state, const int32_t* slots, int n_group, int n_slots, int n,
                             int tok0, int len, int hold_tok, int fade_tok, void* stream);

/* y = gelu_erf(x) elementwise (nn.GELU() in CrossPredictor.ffn). */
int mvq_gelu_f32(const float* x, float* y, size_t n, void* stream);

/* y(b,c,t) = a(b,c,t) - b(b,c,t)   and   y(b,c,t) = a(b,c,t)   on [batch, c, n] views, each tensor with its
 * own (batch, channel) element strides and time stride 1: chunk slicing `zt[..., s:e] - z_pred`,
 * `z_run[..., s:e] = z_hat` (Training/compare_dacvsproposal_5.py:312,319) and the fold/unfold between
 * [B,C,T] and the token-folded [C, B*n] chunk layout. */
int mvq_sub3d_f32(const float* a, size_t a_sb, size_t a_sc, const float* b, size_t b_sb, size_t b_sc,
                  float* y, size_t y_sb, size_t y_sc, int batch, int c, int n, void* stream);
int mvq_copy3d_f32(const float* a, size_t a_sb, size_t a_sc, float* y, size_t y_sb, size_t y_sc,
                   int batch, int c, int n, void* stream);

/* ---- evaluation metrics next to the path ---------------------------------- */

/* align_by_xcorr (Evaluation/dac_vcpwq_proposed6_latency.py:164-202): for every integer shift s in
 * [-max_shift, max_shift] the correlation c(s) = sum(r_seg * e_seg) of two equal-length signals ref[t], est[t]
 * (s<0: ref[-s:], est[:t+s]; s>0: ref[:t-s], est[s:]), each one fp32 fma chain in sample order; best_shift = first
 * maximum in ascending s (strict >, start -1e18).  corr[2*max_shift+1], scratch[2*max_shift+1] int32, best_shift[1]
 * (device).  One launch pair instead of 2*max_shift+1 reductions with a host comparison each. */
int mvq_align_xcorr_f32(const float* ref, const float* est, int t, int max_shift, float* corr, int32_t* scratch,
                        int32_t* best_shift, void* stream);
/* The same for `batch` pairs in ONE launch pair (rows of pitch t; corr / scratch [batch][2*max_shift+1], best_shift[batch]):
 * psnr_3k_aligned_batch (Evaluation/compare_dacvsproposal_5_eval.py:212-223) aligns every item of a batch.  Per item the
 * chains are those of mvq_align_xcorr_f32, so the shifts are identical. */
int mvq_align_xcorr_batch_f32(const float* ref, const float* est, int batch, int t, int max_shift, float* corr, int32_t* scratch,
                              int32_t* best_shift, void* stream);

/* ---- backward w.r.t. the decoder input (weights are frozen in the reference) ----- */

/* Input-gradient of a conv is a conv with a transformed weight image, so it runs on the same MFMA kernels:
 *   forward Conv1d w[Cout,Cin,ks], stride 1:           wp = mvq_conv1d_pack_dgrad_f32(w)            (flip + transpose)
 *   forward ConvTranspose1d w[Cin,Cout,ks], stride s:  wp = mvq_conv_transpose1d_pack_dgrad_f32(w)  (a strided conv)
 * size query: mvq_conv1d_dgrad_packed_floats(cin, cout, ks) with cin = channels of the forward INPUT. */
size_t mvq_conv1d_dgrad_packed_floats(int cin, int cout, int ks);
int mvq_conv1d_pack_dgrad_f32(const float* w, float* wp, int cin, int cout, int ks, void* stream);
int mvq_conv_transpose1d_pack_dgrad_f32(const float* w, float* wp, int cin, int cout, int ks, void* stream);

/* gx[B,cin,tin] = ( dgrad-conv(gy[B,cout,tout]) ) * d snake(dsnake_src)/dx  + residual
 * (cin, tin, cout, tout, ks, stride, dil, pad describe the FORWARD layer: stride 1 for Conv1d, the up-sampling stride
 * for a ConvTranspose1d).  dsnake_src[B,cin,tin] = saved input of the Snake1d in front of the forward layer and
 * dsnake_alpha[cin] its alpha (both NULL: no Snake in front); residual[B,cin,tin] = gradient arriving over a skip
 * connection or NULL.  Chain order: forward output channel ascending, then tap ascending. */
int mvq_conv1d_dgrad_f32(const float* gy, const float* wp_dgrad, const float* dsnake_src, const float* dsnake_alpha,
                         const float* residual, float* gx,
                         int batch, int cin, int tin, int cout, int tout, int ks, int stride, int dil, int pad,
                         void* stream);

/* ---- parameter gradients of the decoder's layers (fine-tuning T_DEC; the reference freezes it) -------------------
 * All fp32, no atomics, nothing allocated or synchronised inside a call; refusals return MVQ_EINVAL before any launch and
 * leave every output untouched.  Checked against float64 autograd (fp32 tolerance), not part of the bit-exact contract.
 *
 * mvq_conv1d_wgrad_f32: gradient of a conv weight, in the torch layout of weight_v, described by the geometry of the
 * FORWARD layer (as mvq_conv1d_dgrad_f32).  gy[B,cout,tout] is the gradient at the conv's output, a[B,cin,tin] its input.
 *   transposed = 0, Conv1d (stride must be 1, tout = tin + 2 pad - dil (ks-1)):
 *       dw[co][ci][k] = sum_b sum_t gy[b][co][t] * a[b][ci][t + k*dil - pad]
 *   transposed = 1, ConvTranspose1d (ks == 2*stride, dil 1, tout = (tin-1) stride - 2 pad + ks + output_padding < stride):
 *       dw[ci][co][k] = sum_b sum_t a[b][ci][t] * gy[b][co][t*stride - pad + k]
 *   terms that index outside a row are 0.  snake_alpha[cin] (or NULL): `a` is the saved INPUT of the Snake1d in front of the
 *   layer and the kernel stages snake(a, alpha) -- the arithmetic of the forward's Snake-on-load (det_snake).
 * Summation contract.  t is the token index of the operand that is read unshifted (gy for a Conv1d, a for a
 * ConvTranspose1d), in chunks of TK tokens (TK = 64; transposed: 64 / 32 / 32 / 16 for stride 2 / 4 / 5 / 8).  The list of
 * (item b ascending, chunk ascending) is cut into `nsplit` contiguous ranges, range s = [n*s/nsplit, n*(s+1)/nsplit).  Inside a
 * range every output element is ONE fp32 fma chain over the tokens in that order (v_mfma_f32_32x32x2_f32); the ranges' partial
 * sums are added in ascending s, ((p0 + p1) + p2) + ...  nsplit = min(number of chunks, ceil(1024 / block tiles), 4096) is a
 * function of the shape alone, so the same inputs give the same bits on every run and every device.  A layer with at most 4
 * rows on the unshifted side (the decoder's final conv, cout = 1) takes a reduction form: chunks of 1024 tokens, each of 256
 * threads one fma chain over its tokens (stride 256) in range order, then a fixed binary tree over the threads, then the ranges.
 * workspace: mvq_conv1d_wgrad_workspace_bytes(same geometry) bytes of device memory, 4-byte aligned (0 when nsplit = 1; NULL
 * is then accepted).  The query returns 0 for a geometry the call refuses. */
size_t mvq_conv1d_wgrad_workspace_bytes(int batch, int cin, int tin, int cout, int tout, int ks, int stride, int dil, int pad,
                                        int transposed);
int mvq_conv1d_wgrad_f32(const float* gy, const float* a, const float* snake_alpha, float* dw, void* workspace,
                         size_t workspace_bytes, int batch, int cin, int tin, int cout, int tout, int ks, int stride, int dil,
                         int pad, int transposed, void* stream);
/* Sums over the items and tokens of a [B,C,T] tensor, per channel: slabs of 2048 tokens of one item in (item, slab) order are cut
 * into G = min(slabs, max(1, 2048 / C)) contiguous ranges; inside a range each of 256 threads chains its tokens (stride 256),
 * a fixed binary tree adds the threads, and the ranges are added in ascending order.  workspace (both calls below):
 * mvq_channel_reduce_workspace_bytes(batch, c, t) bytes, 4-byte aligned.
 *   mvq_snake_bwd_f32: gs = gradient at a Snake1d's OUTPUT, x its saved input ->
 *       gx = gs * d snake(x)/dx + residual   bit for bit the fused epilogue of mvq_conv1d_dgrad_f32 (one device function)
 *       dalpha[c] = sum_{b,t} gs * (x sin(2 alpha x)/(alpha+1e-9) - sin(alpha x)^2/(alpha+1e-9)^2)     (NULL: not computed,
 *       no workspace needed);  residual may be NULL;  gx must not alias an input.
 *   mvq_bias_grad_f32: db[c] = sum_{b,t} gy[b][c][t]. */
size_t mvq_channel_reduce_workspace_bytes(int batch, int c, int t);
int mvq_snake_bwd_f32(const float* gs, const float* x, const float* alpha, const float* residual, float* gx, float* dalpha,
                      void* workspace, size_t workspace_bytes, int batch, int c, int t, void* stream);
int mvq_bias_grad_f32(const float* gy, float* db, void* workspace, size_t workspace_bytes, int batch, int c, int t, void* stream);
/* Backward of w = g * v / ||v|| over the rows (dim 0, both conv kinds) of v[rows][cols]: with n = ||v_r||, s = <dw_r, v_r>
 *   dg[r] = s / n        dv_r = (g_r / n) * (dw_r - (s / n^2) v_r)         (dg or dv may be NULL)
 * One block per row: each of 256 threads chains its columns (stride 256), a fixed binary tree adds the threads. */
int mvq_weight_norm_bwd_f32(const float* dw, const float* v, const float* g, float* dg, float* dv, int rows, int cols, void* stream);

/* Backward of the reference's own trainable modules (CrossPredictor, TokenNorm, tanh*scale; Training/
 * compare_dacvsproposal_5.py:222-244,313-315 under `scaler.scale(total).backward()`, ...:393).  Same addressing as the
 * forward entry points.  Checked against torch autograd (fp32 tolerance), not part of the bit-exact forward contract.
 *   layernorm_c_bwd : gx (may be NULL) and dgamma/dbeta (ACCUMULATED into) from g; stats[2*B*T] scratch (mu, rstd)
 *   gelu_bwd        : gx = g * gelu'(x)
 *   scale_tanh      : y = scale * tanh(u);  _bwd: gu = g*scale*(1-tanh(u)^2), partial[n_partial] block sums of g*tanh(u)
 *                     (their total is d/dscale), n_partial <= 4096
 *   attention_bwd   : gq, gk, gv from g = dL/dctx (Tq, Tk <= 32)
 *   mul_scaled      : out = a*b*scale (nn.Dropout on ctx, ...:242: the keep-mask is drawn by the caller; also its backward)
 *   transpose2d     : out[c][r] = in[r][c]      rowsum: out[r] (+)= sum_c in[r][c]   (weight / bias gradients: the
 *                     weight gradient dW = g x^T over the token axis runs on mvq_conv1d_f32 with K = tokens) */
int mvq_layernorm_c_bwd_f32(const float* x, const float* pe, const float* gamma, const float* g, float* gx,
                            float* dgamma, float* dbeta, float* stats, int batch, int c, int t,
                            size_t stride_b, size_t stride_c, float eps, void* stream);
int mvq_gelu_bwd_f32(const float* x, const float* g, float* gx, size_t n, void* stream);
int mvq_scale_tanh_f32(const float* u, float scale, float* y, size_t n, void* stream);
int mvq_scale_tanh_bwd_f32(const float* u, const float* g, float scale, float* gu, float* partial, int n_partial, size_t n,
                           void* stream);
int mvq_attention_bwd_f32(const float* q, const float* k, const float* v, const float* g, float* gq, float* gk, float* gv,
                          int batch, int heads, int dh, int tq, int tk,
                          size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, void* stream);
/* Backward of mvq_attention_seq_f32 for Tq, Tk <= 512 and dh <= 256 (the 1-, 2- and 4-s PLC training segments): gq, gk,
 * gv from g = dL/dctx, same addressing.  scratch: mvq_attention_seq_bwd_scratch_bytes(batch, heads, tq, tk) bytes of device
 * memory (P and dS, 2*batch*heads*tq*tk floats), 16-byte aligned.  Not bit-exact (checked against float64 autograd). */
size_t mvq_attention_seq_bwd_scratch_bytes(int batch, int heads, int tq, int tk);
int mvq_attention_seq_bwd_f32(const float* q, const float* k, const float* v, const float* g, float* gq, float* gk, float* gv,
                              void* scratch, int batch, int heads, int dh, int tq, int tk,
                              size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, void* stream);
/* Backward under a KEY MASK (kmask as in mvq_attention_masked_f32): gq is, bit for bit, what mvq_attention_bwd_f32 /
 * mvq_attention_seq_bwd_f32 return on the item's K and V compacted to J(b) with Tk = |J(b)|; gk / gv at a present column are
 * that launch's values at the column's slot, and at an absent column they are written as +0 (every output element is
 * defined).  |J(b)| = 0 gives gq = +0 and gk = gv = +0 for that item.  K and V of an absent column never reach any output (NaN
 * or 1e30 there changes nothing): the chunk kernel compacts while it stages, the sequence kernels predicate every chain on
 * presence and never multiply by the mask.  kmask == NULL is the unmasked launch.  Shape limits and refusals (before any
 * launch) are those of mvq_attention_bwd_f32 (Tq, Tk <= 32, 64 KiB of LDS) and mvq_attention_seq_bwd_f32 (Tq, Tk <= 512,
 * dh <= 256); the scratch of the sequence form has the unmasked size. */
int mvq_attention_masked_bwd_f32(const float* q, const float* k, const float* v, const uint8_t* kmask, const float* g,
                                 float* gq, float* gk, float* gv, int batch, int heads, int dh, int tq, int tk,
                                 size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c, size_t m_stride_b,
                                 void* stream);
int mvq_attention_seq_masked_bwd_f32(const float* q, const float* k, const float* v, const uint8_t* kmask, const float* g,
                                     float* gq, float* gk, float* gv, void* scratch, int batch, int heads, int dh, int tq, int tk,
                                     size_t q_stride_b, size_t q_stride_c, size_t k_stride_b, size_t k_stride_c,
                                     size_t m_stride_b, void* stream);
/* Loss pattern of a lossy link for the training step: counts[batch, t] uint8, token tk takes packet tk / packet_tok; 0 = the
 * packet is lost, otherwise the number of books (of nb) that arrive.  Per item a two-state Gilbert-Elliott chain over its packets,
 * drawn from a stateless 32-bit hash of (seed, step, stream_id, item_base + b, packet, draw): pure integer arithmetic, equal bit
 * for bit to packets.channel_counts (which documents the hash and the four draws), and row b depends on item_base + b alone.  The
 * thresholds are min(2^32, int(q * 2^32)) of the probabilities loss, thin, p_gb, p_bg, loss_bad.  One thread walks one item's
 * chain.  Refused before any launch: packet_tok < 1, min_books outside 1..nb, nb outside 1..255, a threshold above 2^32. */
int mvq_channel_draw_u8(uint8_t* counts, int batch, int t, int packet_tok, int nb, int min_books,
                        uint64_t thr_loss, uint64_t thr_thin, uint64_t thr_gb, uint64_t thr_bg, uint64_t thr_loss_bad,
                        uint32_t seed, uint32_t step, uint32_t stream_id, uint32_t item_base, void* stream);
/* Packet-loss fill (PLC/PLC1.py:401-410) on [batch, c, t] tensors with element (b,c,t) at b*stride_b + c*stride_c + t
 * (0,0 = contiguous; stride_b = t, stride_c = batch*t is the token-folded [C, B*T] layout); mask is uint8 [batch, t],
 * contiguous, non-zero = token lost.
 *   zt_in    = zt * (~mask)                    an IEEE multiply by 1 or 0, as torch's: -0 kept, NaN and inf give NaN
 *   z_filled = where(mask, z_pred, zt_in)      either output may be NULL (not written); z_pred may be NULL with z_filled
 *   _bwd: g_zpred = where(mask, g, 0)          torch.where's backward w.r.t. z_pred */
int mvq_plc_mask_fill_f32(const float* zt, const float* z_pred, const uint8_t* mask, float* zt_in, float* z_filled,
                          int batch, int c, int t, size_t stride_b, size_t stride_c, void* stream);
int mvq_plc_mask_fill_bwd_f32(const float* g, const uint8_t* mask, float* g_zpred,
                              int batch, int c, int t, size_t stride_b, size_t stride_c, void* stream);
/* PLC evaluation (PLC/PLC1_eval.py:270-333,601-663, PLC/PLC1_low_mid_high_eval.py:264-288).
 * mvq_frame_subsets: token mask (uint8 [t_lat], non-zero = lost) -> frame_mask uint8 [t_frames] with frame f on token
 *   clip(floor(double(f*hop) / (double(t_wave)/double(t_lat))), 0, t_lat-1) (numpy float64), and the ascending frame indices
 *   of the lost / kept frames in cols_masked / cols_unmasked (t_frames ints each); counts[0..1] = their lengths, on the
 *   device.  t_lat = 0 or t_wave = 0: counts are 0 and frame_mask is all 0.  t_frames <= 32768.
 * mvq_mel_ssim_f32: n images, one block each; image i is described by desc[5i..5i+4] = {x column base, y column base, x max
 *   index, y max index, list offset (-1: columns 0..w-1)} into the mel plane mel [rows = 64, ld] and maxv[n_maxv], and its
 *   width w = widths[i] (device, clamped to [0, max_width]); columns are base + cols[offset + j].  Values are
 *   mel / max(maxv, 1e-8).  mode MVQ_SSIM_SSIM: the 7x7 uniform-window SSIM of skimage's defaults (data_range 1), the mean of
 *   the map cropped by 3; w = 1..6 and mode MVQ_SSIM_NORM: max(0, 1 - |A-B|/(|A|+|B|+1e-12)); w = 0: NaN.  out: double [n].
 *   max_width <= 32768 and rows == 64, else MVQ_EINVAL before any launch.  Deterministic, independent of the other images.
 * mvq_subset_stats_f32: ref, est [t] with sample n on token floor(float(n) / float(t/t_lat)) (token_to_sample_mask);
 *   out double[8] = lost side {count, sum |r-e|, sum r^2, sum (r-e)^2}, then the kept side.  t <= 2^24. */
#define MVQ_SSIM_NORM 0
#define MVQ_SSIM_SSIM 1
int mvq_frame_subsets(const uint8_t* latent_mask, int t_lat, long long t_wave, int hop, int t_frames, uint8_t* frame_mask,
                      int* cols_masked, int* cols_unmasked, int* counts, void* stream);
int mvq_mel_ssim_f32(const float* mel, int rows, size_t ld, const float* maxv, int n_maxv, const int* desc, const int* cols,
                     size_t n_cols, const int* widths, int n, int max_width, int mode, double* out, void* stream);
int mvq_subset_stats_f32(const float* ref, const float* est, long long t, const uint8_t* latent_mask, int t_lat, double* out,
                         void* stream);
int mvq_mul_scaled_f32(const float* a, const float* b, float scale, float* out, size_t n, void* stream);
int mvq_transpose2d_f32(const float* in, float* out, int rows, int cols, void* stream);
int mvq_rowsum_f32(const float* in, float* out, int rows, int cols, int accumulate, void* stream);

/* Training losses: safe_l1, MultiResSTFTLoss, MelCosineLoss of
 * Training/compare_dacvsproposal_5.py:150-211 and their gradient w.r.t. the predicted waveform.  The STFT is a GEMM:
 * frames[n_fft, cols] (windowed, reflect-padded, center=True) times a real DFT basis -> spec[2*fp, cols] on
 * mvq_conv1d_f32 (k = 1), rows [0,f) = Re, rows [fp, fp+f) = Im, f = n_fft/2+1, fp = f rounded up to 32; its gradient is
 * the transposed GEMM followed by overlap_add.  Column = half*batch*nframes + b*nframes + n, half 0 = prediction,
 * half 1 = target, ncols >= 2*batch*nframes, nframes = 1 + t/hop.  These entry points are the HBM-bound glue:
 *   stft_frames       out[f][col0 + b*nframes + n] = window[f] * finite_or_zero(x[b][reflect(n*hop + f - n_fft/2)])
 *   spec_mag          mag[k][c] = max(|spec|, eps)   (rows f..fp-1 zero)
 *   spec_loss_partial partial[3][batch][p]: sums of (X-Y)^2, Y^2, |X-Y| per item (spectral convergence and log-free
 *                     magnitude L1 of MultiResSTFTLoss.forward, ...:166-170)
 *   spec_grad         g[2*fp][batch*nframes] = dL/d(Re,Im) of the prediction from coef_a[b]*(X-Y) + coef_b*sign(X-Y)
 *                     + extra[k][c] (extra: gradient arriving from the mel branch, may be NULL)
 *   overlap_add       dy[b][t] += sum of window*dframes over the frames (and reflections) covering sample t
 *   l1_loss           partial[p] block sums of |y - tgt| (finite_or_zero applied); dy += coef*sign(y - tgt) if dy
 *   mel_max / mel_cos / mel_max_grad : per-item max of the mel spectrogram (MelCosineLoss._mel_mag's amax), the per-frame
 *                     cosine of log(M/max + eps) and its gradient w.r.t. the prediction's mel magnitudes (dmel[n_mels]
 *                     [batch*nframes], dden per column; mel_max_grad routes the max's gradient to its argmax element);
 *                     use_log = 0 gives the cosine of the max-normalised LINEAR mel frames = stsim_batch
 *                     (Evaluation/compare_dacvsproposal_5_eval.py:142-177; forward only)
 * Checked against torch autograd on the restated losses and fixture G7 (fp32 tolerance). */
int mvq_stft_frames_f32(const float* x, const float* window, float* out, int batch, int t, int n_fft, int hop, int nframes,
                        size_t ncols, size_t col0, void* stream);
int mvq_spec_mag_f32(const float* spec, float* mag, int f, int fp, size_t ncols, float eps, void* stream);
int mvq_spec_loss_partial_f32(const float* mag, float* partial, int p, int f, int batch, int nframes, size_t ncols, void* stream);
int mvq_spec_grad_f32(const float* spec, const float* mag, const float* coef_a, float coef_b, const float* extra, float* g,
                      int f, int fp, int batch, int nframes, size_t ncols, float eps, void* stream);
int mvq_overlap_add_f32(const float* dframes, const float* window, float* dy, int batch, int t, int n_fft, int hop, int nframes,
                        void* stream);
int mvq_l1_loss_f32(const float* y, const float* tgt, float* partial, int p, float* dy, float coef, size_t n, void* stream);
int mvq_mel_max_f32(const float* mel, float* maxv, int* argmax, int n_mels, int batch, int nframes, size_t ncols, void* stream);
int mvq_mel_cos_f32(const float* mel, const float* maxv, float* cosv, float* dmel, float* dden, float coef, int n_mels, int batch,
                    int nframes, size_t ncols, float eps, int use_log, void* stream);
int mvq_mel_max_grad_f32(const float* dden, const float* maxv, const int* argmax, float* dmel, int batch, int nframes, float eps,
                         void* stream);

/* Zero-padded rows.  A layer whose natural length is not a multiple of 4 (the decoder's 2 999-sample block) would take
 * the 4-byte load / store paths.  Instead its tensors are allocated with rows rounded up to a multiple of 4 and the tail kept
 * at ZERO, which is exactly the zero padding a conv sees beyond the end of its input: every kernel then runs its 16-byte
 * paths and the results of the true columns are bit-identical.  `tvalid` = true length: output columns >= tvalid are
 * written as zeros (0 = all columns are data).  conv_transpose1d: `tout_rows` = row length of y (0 = natural; smaller when
 * the input carried a zero tail; up to `pad` larger with tvalid <= natural).  MFMA-tiled shapes only. */
int mvq_conv1d_padded_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                          const float* residual, const float* alpha_out, float* y, float* y2, const float* alpha2,
                          int batch, int cin, int tin, int cout, int ks, int stride, int dil, int pad, int act, int tvalid,
                          void* stream);
int mvq_residual_unit_padded_f32(const float* x, const float* x_snaked, const float* w7p, const float* b7,
                                 const float* alpha_a, const float* alpha_b, const float* w1p, const float* b1,
                                 const float* alpha_next, float* y, float* y2, const float* alpha2, float* scratch,
                                 int batch, int c, int t, int dil, int tvalid, void* stream);
int mvq_conv_transpose1d_padded_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                    const float* alpha_out, float* y, float* y2, const float* alpha2,
                                    int batch, int cin, int tin, int cout, int stride, int pad, int tout_rows, int tvalid,
                                    void* stream);
/* The same with torch's ``output_padding`` (0 <= output_padding < stride, <= pad): the natural row length grows by that many
 * samples at the END of each row -- the same sum evaluated there.  For the DecoderBlock variant with
 * ``output_padding = stride % 2`` (believed to be upstream DAC's repository head; release 1.0.0 -- the default of this
 * package and of the oracle -- passes none): 75 tokens then decode to 24 000 samples instead of 23 992. */
int mvq_conv_transpose1d_op_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                const float* alpha_out, float* y, float* y2, const float* alpha2,
                                int batch, int cin, int tin, int cout, int stride, int pad, int output_padding, int tout_rows,
                                int tvalid, void* stream);

/* VIRTUALLY PACKED latent-rate rows (round 4): the same tiling as the packed layout -- seg_per_row items side by side in one
 * GEMM row, so a 128-column tile holds live columns only -- but with NO repacked copy of the input or the output: the LDS-DMA
 * source of every 16-byte piece is remapped (virtual column c -> item c / per_in, position c mod per_in; positions >= tin_rows
 * read zeros) and the epilogue stores column n to (item n / tout_rows, position n mod tout_rows) of the ordinary tensor.
 * Used for the encoder's last strided conv (512 -> 1024, k 16, s 8, T 600 -> 75: 78 % -> 98 % live columns) and the k3 conv
 * behind it (upstream dac Encoder tail; Training/compare_dacvsproposal_5.py:294,296).
 *   x[batch, cin, tin_rows]: tin_valid data columns then a zero tail (caller's contract, as for the zero-padded rows below);
 *   y[batch, cout, tout_rows]: conv_out_len(tin_valid) valid columns, the rest written as zeros.  Requirements: tin_rows,
 *   tout_rows, per_in multiples of 4; per_in == stride * tout_rows; per_in - tin_valid >= max(pad, right overhang of the last
 *   output); no Snake on load (the DMA cannot transform what it copies).  Same fma chains as mvq_conv1d_f32 on each item. */
int mvq_conv1d_vpacked_f32(const float* x, const float* wp, const float* bias, const float* residual, const float* alpha_out,
                           float* y, float* y2, const float* alpha2, int batch, int cin, int tin_rows, int tin_valid, int cout,
                           int ks, int stride, int dil, int pad, int act, int seg_per_row, int per_in, int tout_rows, void* stream);

/* PACKED latent-rate rows (round 3).  At the latent rate a segment is 75 columns wide: one 96- or 128-column tile per segment
 * leaves 22-41 % of the MFMAs on padding.  The decoder's first two layers therefore run on rows that hold `seg_per_row` segments
 * at a period of `seg_period` columns (a multiple of 4), `seg_valid` of them data and the rest ZEROS -- the zero padding each
 * conv would see between neighbours, so every data column is computed exactly as in the unpacked layer (same fma chains).
 *   mvq_conv1d_packed_rows_f32: a stride-1 'same' conv (2*pad == (ks-1)*dil, pad <= seg_period - seg_valid) x[rows,cin,L] ->
 *     y[rows,cout,L], L = seg_per_row * seg_period; gap columns of the output are written as zeros (also in y2).
 *   mvq_conv_transpose1d_packed_rows_f32: ConvTranspose1d(kernel 2*stride, stride, pad) reading such rows and writing the
 *     UNPACKED y[batch_out, cout, (seg_valid-1)*stride - 2*pad + 2*stride]: segment g of row r is batch item r*seg_per_row + g.
 * Replaces nothing new in the reference: it is `T_DEC`'s `model.0` / `model.1.block.1` (Training/compare_dacvsproposal_5.py:322). */
int mvq_conv1d_packed_rows_f32(const float* x, const float* wp, const float* bias, const float* residual, const float* alpha_out,
                               float* y, float* y2, const float* alpha2, int rows, int cin, int cout, int ks, int dil, int pad,
                               int act, int seg_per_row, int seg_period, int seg_valid, void* stream);
int mvq_conv_transpose1d_packed_rows_f32(const float* x, const float* wp, const float* bias, const float* alpha_in,
                                         const float* alpha_out, float* y, float* y2, const float* alpha2, int rows, int cin,
                                         int cout, int stride, int pad, int seg_per_row, int seg_period, int seg_valid,
                                         int batch_out, void* stream);

/* OPT-IN, NON-PARITY arithmetic mode "bf16x6" for the wide ResidualUnits' 7-tap dilated convs (upstream dac ResidualUnit,
 * called through Training/compare_dacvsproposal_5.py:294-296,322): the default path above is an exact k-ordered fp32 fma chain;
 * these three entry points are the one deliberate departure and nothing calls them unless the caller asks for the mode
 * (Python: multimodal_vqvae_compression_audio_tactile_amd.set_arith("bf16x6")).  Every fp32 operand is split into three
 * bf16 pieces (24 significant bits) and a product is six piece products on v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
 * fp32-ACCURATE (the dropped terms are < 2^-24 |ab|) but summed in another order than the contract, so NOT bit-identical to the
 * oracle; it earns no parity claim and is reported as its own bench line (dtype "bf16x6").
 *   mvq_bf16x3_split_f32        x[batch, c, t] fp32 -> xs (mvq_bf16x3_split_bytes bytes): [batch][c/8][3 pieces][t][8] bf16; c % 8 == 0
 *   mvq_conv1d_k7_pack_bf16x3   folded weights w[cout, cin, 7] fp32 -> wq (mvq_conv1d_k7_bf16x3_packed_bytes bytes);
 *                               cout % 128 == 0 or cout % 96 == 0, cin % 16 == 0
 *   mvq_conv1d_k7_bf16x6_f32    y[batch, cout, t] = snake_out(conv7_dil(xs) + bias), 'same' padding 3 * dil, dil in {1, 3, 9};
 *                               xs already carries the input Snake (the producer's dual output); tvalid as for the
 *                               zero-padded rows above (0 = every column is data).
 * Training config (Decoder.forward_saving / backward_input; all optional, NULL otherwise):
 *   y2 != NULL       dual output: y = conv + bias (the pre-activation the backward saves), y2 = snake_out(y) (what the 1x1 conv reads)
 *   pack ... dgrad=1 the INPUT-GRADIENT image of a forward weight w[c, m, 7] (cout = the forward Cin, cin = the forward Cout):
 *                    W'[m][c][k] = w[c][m][6 - k]; the same conv call on the output gradient then is the gradient w.r.t. the input
 *   dsn_src, dsn_alpha, residual   the input-gradient epilogue of mvq_conv1d_dgrad_f32: v = acc * d snake(dsn_src)/dx + residual */
size_t mvq_bf16x3_split_bytes(int batch, int c, int t);
int mvq_bf16x3_split_f32(const float* x, void* xs, int batch, int c, int t, void* stream);
size_t mvq_conv1d_k7_bf16x3_packed_bytes(int cout, int cin);
int mvq_conv1d_k7_pack_bf16x3(const float* w, void* wq, int cout, int cin, int dgrad, void* stream);
int mvq_conv1d_k7_bf16x6_f32(const void* xs, const void* wq, const float* bias, const float* alpha_out, float* y, float* y2,
                             const float* dsn_src, const float* dsn_alpha, const float* residual,
                             int batch, int cin, int t, int cout, int dil, int tvalid, void* stream);

/* The same opt-in departure with TWO fp16 pieces per operand and THREE piece products ("f16x3"): half the matrix work of bf16x6.
 * fp16 has 11 significant bits but a 5-bit exponent, so every ITEM of the activations and the weight tensor are first scaled by
 * the power of two that puts their largest magnitude into [2^13, 2^14) (exact); the scales are kept as the float bit patterns of
 * those maxima (xamax[batch], wamax[1], written by the split / pack calls) and undone in the conv's epilogue.  Error per product
 * <= ~3 x 2^-22 (dropped h1 g1 term + the two representation errors): about twice the rounding error of the exact fp32 chain, i.e.
 * fp32-class; the maxima are taken over the FINITE elements, so a NaN / Inf sample contaminates its own receptive field only (as in
 * the exact path) and does not disturb the item's scale; finite magnitudes above the fp32 range of a S are outside its contract.
 *   mvq_f16x2_split_f32       x[batch, c, t] -> xs (4 bytes per element: [batch][c/8][2 pieces][t][8] fp16), xamax[batch]
 *   mvq_conv1d_k7_pack_f16x2  w[cout, cin, 7] -> wq (mvq_conv1d_k7_f16x2_packed_bytes), wamax[1]
 *   mvq_conv1d_k7_f16x3_f32   as mvq_conv1d_k7_bf16x6_f32 */
int mvq_f16x2_split_f32(const float* x, void* xs, uint32_t* xamax, int batch, int c, int t, void* stream);
size_t mvq_conv1d_k7_f16x2_packed_bytes(int cout, int cin);
int mvq_conv1d_k7_pack_f16x2(const float* w, void* wq, uint32_t* wamax, int cout, int cin, int dgrad, void* stream);
int mvq_conv1d_k7_f16x3_f32(const void* xs, const uint32_t* xamax, const void* wq, const uint32_t* wamax, const float* bias,
                            const float* alpha_out, float* y, float* y2, const float* dsn_src, const float* dsn_alpha,
                            const float* residual, int batch, int cin, int t, int cout, int dil, int tvalid, void* stream);

/* Polyphase sinc resampler: torchaudio.transforms.Resample(orig, new) as the reference
 * calls it on every file (Training/compare_dacvsproposal_5.py:110-113, Evaluation/dac_vcpwq_proposed6_latency.py:151-156).
 * orig/newf are the rates divided by their gcd, kern[newf][ks] the filter bank (ks = 2*width + orig),
 * y[b][n*newf + p] = sum_k kern[p][k] * xpad[b][n*orig + k] with x zero-padded by `width` on the left,
 * len_out <= ceil(newf*len/orig).  One fp32 fma chain per output sample, k ascending (bit-exact vs the oracle). */
int mvq_resample_f32(const float* x, const float* kern, float* y, int batch, int len, int len_out, int orig, int newf,
                     int width, int ks, void* stream);
/* Ragged form (the resample step of psnr_3k_aligned_batch, ...5_eval.py:217-220, after a per-item alignment shift): item b
 * resamples x[b*pitch + off[b] : ... + len[b]]; off / len are DEVICE int32 arrays (they are computed from the device-side
 * shifts, so no host round trip sits between aligning and resampling).  y rows have pitch lout_pitch; samples at and past
 * ceil(newf*len[b]/orig) are written as zeros and that length goes to len_out[b] (may be NULL).  Same chains as above.
 * A slice is clamped to its row on the device (0 <= off, off + len <= pitch) and to lout_pitch output samples. */
int mvq_resample_ragged_f32(const float* x, const float* kern, float* y, const int32_t* off, const int32_t* len, int32_t* len_out,
                            int batch, int pitch, int lout_pitch, int orig, int newf, int width, int ks, void* stream);

/* ---- streaming receiver: session state in fixed device buffers, updated in place by the kernel ----
 * mvq_resample_stream_f32: mvq_resample_f32 fed piece by piece, for pure decimation (newf == 1 after the gcd; anything else is
 * MVQ_EUNSUPPORTED).  `consumed` = samples of the item given to earlier calls (a multiple of orig), x_new[batch, n_new] the next
 * piece; n_new must be a multiple of orig unless `final` (MVQ_EINVAL).  The call writes y[batch, len_out], the outputs
 * n in [done(consumed), done(consumed + n_new)) of the whole-signal resample, done(L) = max(0, L/orig - hold),
 * hold = ceil(width/orig): output n reads xpad[n*orig .. n*orig + ks), complete once sample n*orig + ks - width - 1 has arrived
 * (24 kHz -> 3 kHz: orig 8, width 49, ks 106: sample 8n + 56).  final = 1 pads zeros on the right and flushes up to
 * ceil((consumed + n_new)/orig).  len_out must equal that count (MVQ_EINVAL: the message names it).
 * STATE LAYOUT: state[batch, S] fp32, S = hold*orig + width (105 for 24 -> 3 kHz; S <= 1024, else MVQ_EUNSUPPORTED), row b holds the
 * last S samples of (zeros | x received so far), oldest first; a new session starts from all zeros (the `width` zeros of the
 * left padding and hold*orig samples no output reads).  The kernel moves it up by n_new samples after the outputs are written
 * (one block per item, a barrier between).  Every output is the fma chain of mvq_resample_f32 (k ascending, the taps that fall
 * on padding skipped): concatenated, the pieces equal the whole-signal call bit for bit.  With consumed >= S and a fixed n_new the
 * launch does not depend on `consumed`, so a captured steady step replays. */
int mvq_resample_stream_f32(const float* x_new, const float* kern, float* state, float* y, int batch, int n_new, long long consumed,
                            int final, int len_out, int orig, int newf, int width, int ks, void* stream);
/* mvq_resample_stream_rational_f32: mvq_resample_f32 fed piece by piece for ANY ratio orig : newf, with the
 * lag chosen by the caller.  A filter block is orig input samples and newf outputs; block q reads xpad[q*orig .. q*orig + ks) and is
 * complete once sample q*orig + width + orig - 1 has arrived.  `hold` >= ceil(width/orig) is the lag in blocks: after L samples (a
 * multiple of orig) the calls have written the blocks q < max(0, L/orig - hold), that is newf * max(0, L/orig - hold) outputs, and the
 * call with final = 1 pads zeros on the right and writes the rest, up to output ceil(newf*(consumed + n_new)/orig): its last block may
 * be partial in its inputs and in its outputs.  len_out must equal the count of the call (MVQ_EINVAL: the message names it).
 * hold = ceil(width/orig) is the smallest lag (with newf == 1 then mvq_resample_stream_f32's outputs and state exactly); a larger one
 * aligns the pieces with something else: the native-rate sender passes the blocks of one 320-sample token at 24 kHz (4 for
 * 44.1 kHz, 40 for 3 kHz), so every call completes whole tokens.
 * STATE LAYOUT: state[batch, S] fp32, S = hold*orig + width (600 for 44.1 -> 24 kHz at hold 4, 47 for 3 -> 24 kHz at hold 40;
 * S <= 1024, else MVQ_EUNSUPPORTED), row b holds the last S samples of (zeros | x received so far), oldest first; a new session starts
 * from all zeros.  The kernel moves it up by n_new samples after the outputs are written (one block per item, a barrier between).
 * kern[newf][ks] is the bank of mvq_resample_f32 (ks = 2*width + orig); every output is that call's fma chain (k ascending, the taps
 * on padding skipped): concatenated, the pieces equal the whole-signal call bit for bit.  With consumed >= S and a fixed n_new the launch
 * does not depend on `consumed`.  MVQ_EINVAL before any launch on ks != 2*width + orig, a negative size, hold < ceil(width/orig),
 * consumed or a non-final n_new that is no multiple of orig, a wrong len_out, or a null pointer with a non-empty shape; batch = 0
 * returns MVQ_OK without a launch. */
int mvq_resample_stream_rational_f32(const float* x_new, const float* kern, float* state, float* y, int batch, int n_new,
                                     long long consumed, int final, int len_out, int orig, int newf, int width, int ks, int hold,
                                     void* stream);
/* mvq_stream_window_f32: the decoder window of a session.  hist[batch, c, cap] (row pitch cap, the first h_in columns valid) and
 * z_new[batch, c, n] (contiguous) -> win[batch, c, h_in + n] = [hist | z_new] (contiguous, a buffer of its own), then
 * hist <- the last h_out columns of win, all in ONE launch: a block owns 32 (b, c) rows, reads them completely, and rewrites only
 * them after a barrier, so the in-place update has no cross-block hazard.  MVQ_EINVAL before any launch on h_out > h_in + n,
 * h_in or h_out > cap, a negative size, or a null pointer with a non-empty shape. */
int mvq_stream_window_f32(float* hist, int h_in, const float* z_new, int n, float* win, int h_out, int cap, int batch, int c,
                          void* stream);
/* mvq_stream_stage_window_f32: the window of one STAGE of the stateful streaming decoder:
 * mvq_stream_window_f32 with the new columns taken from a SLICE of a wider tensor, so the crop of the producer's inexact edges and
 * the window build are one pass.  src[batch, c, src_t] (row pitch src_t); the stage's tail of session b is the [c, cap] block at
 * tail + b * tail_stride (tail = the session state + the stage's fixed offset, tail_stride = the floats of one session's state).
 *   win[b, ch, 0 .. win_t) = [tail[0 .. h_in) | src[b, ch, src_off .. src_off + n) | zeros]   (win_t >= h_in + n: a zero tail keeps the
 *                                                                                            consumer's rows a multiple of 4)
 *   tail[0 .. h_out)       = the last h_out columns of [tail | new]
 * in ONE launch under mvq_stream_window_f32's ownership rule (a block reads its (b, ch) rows completely and rewrites only them
 * after a barrier).  16-byte loads and stores when h_in, n, h_out, cap, src_t, src_off, win_t and tail_stride are multiples of 4
 * and the pointers 16-byte aligned, 4-byte ones otherwise; no atomics, no scratch.  Tail columns at and past h_out keep their
 * values.  MVQ_EINVAL before any launch on h_out > h_in + n, h_in or h_out > cap, src_off + n > src_t, win_t < h_in + n,
 * tail_stride < c * cap, a negative size, or a null pointer with a non-empty shape; batch = 0, c = 0 or h_in + n = 0 returns
 * MVQ_OK without a launch (win is then not written).
 * src_seg / win_seg = 1: dense rows, as above.  > 1 (at most 64): PACKED latent-rate rows (below): item b is segment b % seg of
 * row b / seg, src_t / win_t then being the segment period and a row seg * period columns -- what mvq_conv1d_packed_rows_f32 reads
 * and writes, so a stage window can be built from a packed producer into packed rows for a packed consumer.  Only the segments
 * of the batch's own items are written: with batch % win_seg != 0 the caller zeroes the last row's spare segments.
 * mvq_stream_stage_window_slots_f32: the same kernel body with session g of the group on the state row slots[g] of a pool of
 * n_slots rows (the receiver pool's rules below: a slot outside [0, n_slots) reads as zeros and stores nothing; n_group = 0
 * returns MVQ_OK without a launch). */
int mvq_stream_stage_window_f32(float* tail, size_t tail_stride, int h_in, const float* src, int src_t, int src_seg, int src_off, int n,
                                float* win, int win_t, int win_seg, int h_out, int cap, int batch, int c, void* stream);
int mvq_stream_stage_window_slots_f32(float* tail, size_t tail_stride, const int32_t* slots, int n_group, int n_slots, int h_in,
                                      const float* src, int src_t, int src_seg, int src_off, int n, float* win, int win_t, int win_seg,
                                      int h_out, int cap, int c, void* stream);
/* mvq_stream_stage_window_snake_f32 / _slots_f32: the stage window of a WIDE block of the stateful streaming ENCODER (DESIGN.md
 * section 24).  The same body on dense rows (no packed forms) with a second output beside win:
 *   win_s[b, ch, j] = det_snake(win[b, ch, j], alpha[ch], 1.0f / (alpha[ch] + 1e-9f))   for j < h_in + n, +0 in the zero tail,
 * the function and the reciprocal expression of the conv epilogues' dual output, so win_s is bit for bit the Snake copy the
 * producer of a whole-signal encode writes beside its raw output.  The tail stays RAW (a snaked tail would double the state).
 * win_s[batch, c, win_t] has win's layout, alpha[c].  The checks, the ownership rule, the 16-byte / 4-byte choice (win_s must be
 * aligned too) and the slot rules are mvq_stream_stage_window_f32's; no atomics, no LDS, no scratch. */
int mvq_stream_stage_window_snake_f32(float* tail, size_t tail_stride, int h_in, const float* src, int src_t, int src_off, int n, float* win,
                                      float* win_s, const float* alpha, int win_t, int h_out, int cap, int batch, int c, void* stream);
int mvq_stream_stage_window_snake_slots_f32(float* tail, size_t tail_stride, const int32_t* slots, int n_group, int n_slots, int h_in,
                                            const float* src, int src_t, int src_off, int n, float* win, float* win_s, const float* alpha,
                                            int win_t, int h_out, int cap, int c, void* stream);
/* mvq_stream_samples_f32: the sample state of a streaming SENDER session.  buf[rows, cap] fp32 (row pitch
 * cap, the first `fill` samples of every row valid; rows = the audio rows then the tactile rows, so one launch serves both
 * modalities) and x_new[rows, n] (contiguous).  Per row, with v = [buf[0 .. fill) | x_new[0 .. n)]:
 *   win[0 .. w) = v[0 .. w)                  win[rows, w] contiguous, a buffer of its own: what the encoder stacks read
 *   buf[0 .. fill + n - drop) = v[drop ..)    the samples the next window still needs, moved to the front
 * in ONE launch, one block per row: the move overlaps itself, so a block carries its row through registers tile by tile across
 * a barrier and no row is touched by two blocks.  w = 0 and drop = 0 is the pure append.  Columns of buf at and past the new fill
 * are left as they were.  MVQ_EINVAL before any launch on a negative argument, fill > cap, fill + n - drop > cap, w > fill + n,
 * drop > fill + n, or a null pointer with a non-empty shape; rows = 0 (or n = w = drop = 0) returns MVQ_OK without a launch. */
int mvq_stream_samples_f32(float* buf, int fill, const float* x_new, int n, float* win, int w, int drop, int cap, int rows,
                           void* stream);

/* ---- receiver pool: the state of n_slots independent sessions in ONE set of buffers, one row block per
 * slot -- carry[n_slots, c], hist[n_slots, c, cap], state[n_slots, S] -- and a launch serves the n_group sessions that a DEVICE
 * list slots[n_group] (int32) names, in that order; every other tensor of a call is dense over the group.  The caller passes
 * distinct slots inside [0, n_slots): two equal entries would make two blocks update one row.  The kernels check the range
 * themselves as a second line: a slot outside [0, n_slots) reads as zeros and nothing is stored to the pool for it.  All three:
 * MVQ_EINVAL before any launch on a negative size, n_group > n_slots, n_group * c beyond 2^31 - 1 or a null pointer with a
 * non-empty shape; n_group = 0 returns MVQ_OK without a launch.  The window and the resampler run the kernel body of their dense
 * entry point under this addressing (one template, two instantiations), behind the same argument check.
 * mvq_stream_window_slots_f32: mvq_stream_window_f32 with row (g, ch) of z_new[n_group, c, n] and win[n_group, c, h_in + n] on
 * hist[slots[g]][ch]; the other refusals of mvq_stream_window_f32.  Rows of unlisted slots are not touched.
 * mvq_resample_stream_slots_f32: mvq_resample_stream_f32 with item g of x_new[n_group, n_new] and y[n_group, len_out] on
 * state[slots[g]]; same fma chain, same refusals.  `consumed` names the group's launch class: the launch depends on it only
 * through base = max(0, hold*orig - consumed), lead = max(0, S - consumed) and the output count, which agree for all sessions
 * with consumed == 0 and, n_new and final given, for all with consumed >= S; a value in (0, S) is refused (MVQ_EINVAL).
 * mvq_stream_rows_f32: rows[g][0 .. c) <- pool[slots[g]][0 .. c) (scatter == 0), or pool[slots[g]] <- rows[g] (scatter != 0). */
int mvq_stream_window_slots_f32(float* hist, const int32_t* slots, int n_group, int n_slots, int h_in, const float* z_new, int n,
                                float* win, int h_out, int cap, int c, void* stream);
int mvq_resample_stream_slots_f32(const float* x_new, const float* kern, float* state, const int32_t* slots, int n_group, int n_slots,
                                  float* y, int n_new, long long consumed, int final, int len_out, int orig, int newf, int width, int ks,
                                  void* stream);
int mvq_stream_rows_f32(float* pool, const int32_t* slots, int n_group, int n_slots, float* rows, int c, int scatter, void* stream);
/* mvq_resample_stream_rational_slots_f32: mvq_resample_stream_rational_f32 on the sessions slots[n_group] of a pool state[n_slots, S],
 * as mvq_resample_stream_slots_f32 is to mvq_resample_stream_f32: item g of x_new[n_group, n_new] and y[n_group, len_out] on
 * state[slots[g]], the same kernel body, the same refusals and those of the pool calls above; `consumed` names the group's launch
 * class, 0 or at least S (a value in (0, S) is MVQ_EINVAL). */
int mvq_resample_stream_rational_slots_f32(const float* x_new, const float* kern, float* state, const int32_t* slots, int n_group,
                                           int n_slots, float* y, int n_new, long long consumed, int final, int len_out, int orig,
                                           int newf, int width, int ks, int hold, void* stream);
/* mvq_resample_stream_rational_split_f32 / _split_slots_f32: the SPLIT form of the two calls above -- the same
 * arguments, the same refusals with the same codes, the same outputs and the same state afterwards, bit for bit, in two launches
 * on the one stream.  The outputs launch spreads a session's outputs over a grid of (parts, sessions) blocks, each a range of
 * phases by a range of filter blocks, which read [state | x_new] and write y only; the state launch, one block per session, then
 * moves the state up by n_new samples.  One session's piece no longer waits on the serial work of one block: the form for few
 * sessions.  len_out = 0 leaves the first launch out, n_new = 0 the second. */
int mvq_resample_stream_rational_split_f32(const float* x_new, const float* kern, float* state, float* y, int batch, int n_new,
                                           long long consumed, int final, int len_out, int orig, int newf, int width, int ks, int hold,
                                           void* stream);
int mvq_resample_stream_rational_split_slots_f32(const float* x_new, const float* kern, float* state, const int32_t* slots, int n_group,
                                                 int n_slots, float* y, int n_new, long long consumed, int final, int len_out, int orig,
                                                 int newf, int width, int ks, int hold, void* stream);
/* mvq_stream_samples_slots_f32: the sample state of a group of SENDER sessions of a pool: the kernel body of
 * mvq_stream_samples_f32 under the slot addressing, with fill, n and drop PER SESSION.  buf[n_slots, 2, cap] fp32: slot s owns row 2s
 * (audio) and row 2s + 1 (tactile).  desc[n_group][5] int32 on the DEVICE, per session (slot, fill, n, drop, x_off): its n new audio
 * samples lie at x_new[x_off], its n new tactile samples at x_new[x_off + n]; x_new is ONE packed array of x_total floats (the
 * caller lays the sessions out one after the other: x_off = the exclusive prefix sum of 2n).  win[2, n_group, w] contiguous, a
 * buffer of its own: the audio rows of all sessions, then the tactile rows; w is one value per launch.  Per session and modality,
 * exactly what mvq_stream_samples_f32 does for a row: win = the first w samples of [buf | new], buf <- [buf | new] from drop on.
 * ONE launch of 2 * n_group blocks, one per row; rows of unlisted slots are not touched, nor the columns past a row's new fill.
 * w = 0 with every drop = 0 is the pure append.  The caller passes distinct slots and, per session, values mvq_stream_samples_f32
 * accepts for that w; the kernel checks them itself as a second line: for a descriptor with a slot outside [0, n_slots), a
 * negative value, n > 2^24, fill > cap, drop > fill + n, fill + n - drop > cap, w > fill + n or x_off + 2n > x_total both window
 * rows of the session are written as zeros and nothing is stored to the pool.  MVQ_EINVAL before any launch on a negative size,
 * cap > 2^24, n_group > n_slots or a null pointer with a non-empty shape; n_group = 0 returns MVQ_OK without a launch. */
int mvq_stream_samples_slots_f32(float* buf, const int32_t* desc, int n_group, int n_slots, const float* x_new, int x_total, float* win,
                                 int w, int cap, void* stream);

/* Optimiser step of the training config (torch.optim.AdamW + clip_grad_norm_, Training/compare_dacvsproposal_5.py:367,394-395):
 *   sumsq_partial : partial[n_partial] block sums of x^2 (their total is the squared gradient norm), n_partial <= 4096
 *   adamw         : decoupled-weight-decay Adam on one tensor, torch's single-tensor operation order; clip_coef (device,
 *                   may be NULL) multiplies the gradient on the fly; `step` is the 1-based step count (bias corrections). */
int mvq_sumsq_partial_f32(const float* x, float* partial, int n_partial, size_t n, void* stream);
int mvq_adamw_f32(float* p, const float* g, float* m, float* v, const float* clip_coef, size_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int step, void* stream);

/* out = g * (1 - y*y): backward of the decoder's final tanh (y = saved output). */
int mvq_mul_dtanh_f32(const float* g, const float* y, float* out, size_t n, void* stream);

/* ---- whole stacks (encoder_fwd, decoder_fwd, decoder_bwd_input) ------------------------------------------
 * One call per stack instead of one per layer: `A_ENC(a)` / `T_ENC(t)` (Training/compare_dacvsproposal_5.py:294,296), `T_DEC(z)`
 * (...:322) and the gradient of T_DEC w.r.t. its input under `scaler.scale(total).backward()` (...:393; weights frozen, ...:283-284).
 *
 * A stack handle holds the launch plan and pointers into a caller-provided WEIGHTS BLOB in which mvq_*_create folds the weight norm
 * and packs every conv once (for a decoder also the input-gradient images), next to copies of the biases and Snake alphas.  The
 * parameters are handed over as device pointers in the order mvq_stack_param_info() reports -- upstream `dac` state-dict names
 * ("block.1.block.0.block.1.weight_v", "model.3.block.1.bias", ...) with their shapes -- so any caller that can read a checkpoint
 * can bind them; they are not referenced after create returns.  create with params == NULL and weights_blob == NULL makes a
 * description-only handle (param_info / weights_bytes / out_len / workspace queries work, fwd does not).
 *
 * A forward / backward call walks the plan the Python mirror used to hold: dual outputs (a producer also emits the Snake its wide
 * consumer needs), one fused launch per ResidualUnit of width 64 / 96 / 128, zero-padded rows where a length is not a multiple of
 * 4, and at throughput batch sizes the virtually packed (encoder tail) / packed (decoder head) latent-rate rows.  Intermediates
 * live in a caller-provided WORKSPACE (mvq_*_workspace_bytes, laid out by a deterministic first-fit arena); nothing is allocated
 * or synchronised, so a call can be captured into a hipGraph.  A call sizes its plan before it enqueues anything: a workspace
 * smaller than the plan needs (at most the matching query) is refused with MVQ_EINVAL and nothing is launched -- also when the
 * query was made before mvq_stack_set_plan changed the thresholds.  Results are bit-identical to the per-layer entry points above
 * (tests/test_gpu_stacks.py) and to oracle/c/oracle.c.
 *
 *   mvq_encoder_fwd_f32        x[batch, 1, t]            -> z[batch, d_latent, mvq_encoder_out_len(t)]
 *   mvq_decoder_fwd_f32        z[batch, input_channel, t] -> y[batch, d_out, mvq_decoder_out_len(t)]  (tanh applied)
 *   mvq_decoder_fwd_saving_f32 the same values, keeping every Snake input and the output in `saved` (mvq_decoder_saved_bytes)
 *   mvq_decoder_bwd_input_f32  gz[batch, input_channel, t] = dL/dz from gy = dL/dy and `saved`: the same MFMA conv kernels on flipped /
 *                              transposed weight images with the Snake and tanh derivatives in their epilogues (bit-identical to
 *                              mvq_conv1d_dgrad_f32 layer by layer)
 * mvq_stack_set_plan: batch thresholds of the packed latent-rate forms (0 = keep; defaults 32 / 32) -- A/B measurements only. */
typedef struct mvq_stack mvq_stack;
typedef struct mvq_encoder_desc { int d_model; int n_strides; int strides[8]; int d_latent; } mvq_encoder_desc;     /* dac Encoder(64, [2,4,5,8], 1024) */
typedef struct mvq_decoder_desc { int input_channel; int channels; int n_rates; int rates[8]; int d_out; int output_padding; } mvq_decoder_desc;
int mvq_encoder_create(mvq_stack** out, const mvq_encoder_desc* desc, const float* const* params, void* weights_blob, size_t blob_bytes, void* stream);
int mvq_decoder_create(mvq_stack** out, const mvq_decoder_desc* desc, const float* const* params, void* weights_blob, size_t blob_bytes, void* stream);
void mvq_stack_destroy(mvq_stack* s);
int mvq_stack_param_count(const mvq_stack* s);
int mvq_stack_param_info(const mvq_stack* s, int i, char* name, int name_len, int* dims3);
size_t mvq_stack_weights_bytes(const mvq_stack* s);
int mvq_stack_set_plan(mvq_stack* s, int vpack_min_batch, int pack_min_batch);
int mvq_encoder_out_len(const mvq_stack* s, int t);
size_t mvq_encoder_workspace_bytes(const mvq_stack* s, int batch, int t);
int mvq_encoder_fwd_f32(const mvq_stack* s, const float* x, float* z, void* workspace, size_t workspace_bytes, int batch, int t, void* stream);
/* Stateful streaming encode: A_ENC / T_ENC piece by piece, every stage -- block.0 (k7), each EncoderBlock,
 * the final Snake + k3 -- keeping the tail of its own input in a per-session state row, so a step encodes only the samples that
 * were not encoded yet instead of a 32-token window for 16 tokens.  Fed the pieces of a signal (calls with any n <= 2^20 - 256 samples,
 * then ONE call with last != 0 and the remaining n >= 0 samples) the emitted latent columns are, per call, those whose receptive
 * field [320 j - 2501, 320 j + 2812] lies inside the samples so far (clamped at the signal's edges; everything left with `last`),
 * and concatenated they equal mvq_encoder_fwd_f32 of the whole signal bit for bit: a stage's window starts on a global column
 * that is a multiple of its stride, and only output columns whose inputs are exact are handed on.
 *   mvq_encoder_stream_plan            host arithmetic only (no device call; works on a description-only handle).  stages ==
 *                                      NULL: -> the stage count.  Else stages[count][5] = (h_in, src_off, n_new, h_out, cap) per
 *                                      stage -- its window is [h_in tail columns | columns [src_off, src_off + n_new) of its
 *                                      producer's output], the last h_out of it are kept -- and emit[2] = the GLOBAL latent
 *                                      columns [t0, t1) the step emits (z_len = t1 - t0; they are the columns [src_off', src_off' +
 *                                      z_len) of the k3 conv's output, src_off' = what a further stage would be handed); -> the
 *                                      stage count, or a negative status.
 *   mvq_encoder_stream_state_floats    floats of one session's state: the RAW stage tails [cin, cap] one after the other (the k3
 *                                      stage's holds values that carry the final Snake, as its producer writes them).  A new
 *                                      session needs no clearing: it reads no tail.
 *   mvq_encoder_stream_workspace_bytes the workspace of the call below for these arguments
 *   mvq_encoder_stream_fwd_f32         state[n_slots, state_floats]; slots == NULL: session g is row g, else row slots[g] (int32 on
 *                                      the device, distinct); x_new[n_group, 1, n] -> z[n_group, d_latent, z_len], the state moved
 *                                      on in place.  Per stage ONE stage-window launch (mvq_stream_stage_window_f32, or _snake_f32
 *                                      in front of a block of 65 channels or more, which needs its input raw and snaked) and then
 *                                      the launches mvq_encoder_fwd_f32 issues for that stage, on dense rows at every batch size.
 *                                      z_len must be t1 - t0 of the plan and the workspace large enough: MVQ_EINVAL otherwise,
 *                                      before any launch. */
int mvq_encoder_stream_plan(const mvq_stack* s, long long samples_before, int n, int last, int32_t* stages, int stages_cap, long long* emit);
size_t mvq_encoder_stream_state_floats(const mvq_stack* s);
size_t mvq_encoder_stream_workspace_bytes(const mvq_stack* s, int n_group, long long samples_before, int n, int last);
int mvq_encoder_stream_fwd_f32(const mvq_stack* s, float* state, const int32_t* slots, int n_group, int n_slots, const float* x_new, int n,
                               long long samples_before, int last, float* z, int z_len, void* workspace, size_t workspace_bytes, void* stream);
int mvq_decoder_out_len(const mvq_stack* s, int t);
size_t mvq_decoder_workspace_bytes(const mvq_stack* s, int batch, int t);      /* covers fwd, fwd_saving and bwd_input */
int mvq_decoder_fwd_f32(const mvq_stack* s, const float* z, float* y, void* workspace, size_t workspace_bytes, int batch, int t, void* stream);
/* Stateful streaming decode: T_DEC piece by piece, every stage -- model.0, each DecoderBlock, the final conv --
 * keeping the tail of its own input in a per-session state row instead of decoding a 36-token window for 16 tokens.  Fed the
 * pieces of a sequence (pushes of any n <= 1024, then ONE call with last != 0 and the remaining n >= 0 tokens), the emitted pieces are
 * those of the window schedule -- samples [320 * (N' - 10), 320 * (N - 10)) clamped at 0 for a step from N' to N tokens, up to
 * 320 * T - 8 with `last` -- and concatenated they equal mvq_decoder_fwd_f32 of the whole sequence bit for bit: no conv kernel's
 * result depends on column position or row length, and a stage computes only columns whose receptive field lies inside its window
 * or at a true sequence edge.  Decoders with rates whose emit range the 10-token rule covers and without output_padding;
 * otherwise MVQ_EUNSUPPORTED.
 *   mvq_decoder_stream_plan            host arithmetic only (no device call; works on a description-only handle): the stages of
 *                                      the step that takes n tokens after tokens_before.  stages == NULL: -> the stage count.
 *                                      Else stages[count][5] = (h_in, src_off, n_new, h_out, cap) per stage -- its window is
 *                                      [h_in tail columns | columns [src_off, src_off + n_new) of its producer's output], the last
 *                                      h_out of it are kept, cap = the tail's capacity -- and emit[2] = the [e0, e1) of the final
 *                                      conv's output that is emitted; -> the stage count, or a negative status.
 *   mvq_decoder_stream_state_floats    floats of one session's state: the stage tails [cin, cap] one after the other (the block
 *                                      tails hold values that carry the block's leading Snake already, as the producer writes
 *                                      them).  A new session needs no clearing: it reads no tail (h_in = 0 everywhere).
 *   mvq_decoder_stream_workspace_bytes the workspace of the call below for these arguments
 *   mvq_decoder_stream_fwd_f32         state[n_slots, state_floats]; slots == NULL: session g is row g (n_group <= n_slots), else
 *                                      row slots[g] (int32 on the device, distinct, the receiver pool's rules);
 *                                      z_new[n_group, input_channel, n] -> y[n_group, d_out, y_len], the state moved on in place.
 *                                      Per stage ONE mvq_stream_stage_window launch, then the launches of mvq_decoder_fwd_f32 for
 *                                      that stage on the window; at the batch sizes where mvq_decoder_fwd_f32 runs its head on
 *                                      PACKED latent-rate rows this call does too (the windows of model.0 and of the first
 *                                      transposed conv are built in packed rows).  All tokens_before >= 16 give the same launch
 *                                      sequence, so the steady step can be captured.  y_len must be e1 - e0 of the plan and the
 *                                      workspace large enough: MVQ_EINVAL otherwise, before any launch. */
int mvq_decoder_stream_plan(const mvq_stack* s, int tokens_before, int n, int last, int32_t* stages, int stages_cap, int32_t* emit);
size_t mvq_decoder_stream_state_floats(const mvq_stack* s);
size_t mvq_decoder_stream_workspace_bytes(const mvq_stack* s, int n_group, int tokens_before, int n, int last);
int mvq_decoder_stream_fwd_f32(const mvq_stack* s, float* state, const int32_t* slots, int n_group, int n_slots, const float* z_new, int n,
                               int tokens_before, int last, float* y, int y_len, void* workspace, size_t workspace_bytes, void* stream);
size_t mvq_decoder_saved_bytes(const mvq_stack* s, int batch, int t);
int mvq_decoder_fwd_saving_f32(const mvq_stack* s, const float* z, float* y, void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes,
                               int batch, int t, void* stream);
int mvq_decoder_bwd_input_f32(const mvq_stack* s, const void* saved, size_t saved_bytes, const float* gy, float* gz, void* workspace,
                              size_t workspace_bytes, int batch, int t, void* stream);

/* ---- the auto-regressive chunk loop as ONE launch ------------------------------------------------------------------------------
 * `for s in range(0, Tlat, AR_CHUNK_TOK)` of AllPredAR.forward_step (Training/compare_dacvsproposal_5.py:302-320) ==
 * ProposedEval.encode_latents (Evaluation/dac_vcpwq_proposed6_latency.py:461-477) under no_grad: per 16-token chunk the
 * CrossPredictor on the shift-by-one input, tanh(TokenNorm(zt - z_pred)) * clamp(scale), proj_down, ResidualVQEMA, proj_up, and the
 * write into z_run that the next chunk's predictor reads.  One persistent kernel (csrc/ar_fused.hip): the stages of every chunk
 * are separated by a grid-wide barrier instead of a launch boundary; each stage runs the arithmetic of the stand-alone entry points
 * above (mvq_layernorm_c_sub_f32, mvq_conv1d_f32 with k = 1, mvq_attention_f32, mvq_rvq_ema_forward_f32), so results are
 * bit-identical to the launch-per-stage sequence.  Launched cooperatively (the grid must be resident at once; the barrier gives up
 * after a bounded wait and mvq_ar_check reports it).  Shapes: the reference's (c_lat 1024, FFN 2048, 8 heads, code dim 96, chunks of
 * 16 tokens, K <= 512).  Linear weights are the packed images of mvq_conv1d_pack_f32 (k = 1); k_all / v_all are the audio keys /
 * values of ALL chunks, token-folded [c_lat][batch * t_audio] (column b * t_audio + t) as the per-chunk calls use them
 * (PosEnc restarts per chunk); pe[16][c_lat]; books [books_use][rvq_k][96].  z_run [batch, c_lat, t_lat] is written chunk by chunk;
 * r_tokens [batch, 96, t_lat] (the tokens ema_step sees) and idx_out [books_use, batch, t_lat] (int32) are optional. */
typedef struct mvq_ar_args {
    int batch, t_lat, t_audio, tactile_only, books_use, rvq_k, c_lat, c_ff, code_dim, heads, chunk;
    float ln_eps, tok_eps, scale;
    const float *zt, *k_all, *v_all, *pe;
    const float *lnq_g, *lnq_b, *wq, *wo, *lnf_g, *lnf_b, *w1, *b1, *w3, *b3;      /* CrossPredictor: ln_q, q_proj, out, ffn[0], ffn[1], ffn[3] */
    const float *tok_g, *tok_b, *wd, *bd, *wu, *bu, *books;                       /* TokenNorm, proj_down, proj_up, vq.books */
    float *z_run, *r_tokens;
    int32_t* idx_out;
} mvq_ar_args;
size_t mvq_ar_workspace_bytes(int batch, int t_lat);
int mvq_ar_latents_f32(const mvq_ar_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* the same loop as stream-ordered stand-alone launches from one host call (batch <= 8; capturable; same bits) */
int mvq_ar_latents_staged_f32(const mvq_ar_args* args, void* workspace, size_t workspace_bytes, void* stream);
/* the staged loop on a PIECE of a longer sequence (a whole number of chunks, the last may be shorter): z_prev[batch, c_lat] (may be
 * NULL = zero) is the last z_run token of the piece before, fed as column 0 of the first chunk's shift-by-one input; the piece's
 * own last token is copied to z_last_out[batch, c_lat] (may be NULL, may be the z_prev buffer).  Pieces run one after the other give
 * the bits of the whole-sequence call.  Not with tactile_only (MVQ_EINVAL). */
int mvq_ar_latents_staged_carry_f32(const mvq_ar_args* args, const float* z_prev, float* z_last_out, void* workspace,
                                    size_t workspace_bytes, void* stream);
/* mvq_ar_latents_staged_carry_f32 with closed-loop rate control (mvq_rvq_rate_f32's rule and argument checks, group = the 16-token
 * chunk): one rate launch per chunk after the search; z_run is built from the books each packet carries, in the receiver's
 * arithmetic, and so equals the receiver's bit for bit.  Also writes nb_valid_out[batch, t_lat] and nb_sent_out[batch,
 * ceil(t_lat / packet_tok)].  args->idx_out is required; z_prev / z_last_out as in the carry form (both may be NULL).  Same bits
 * as the launch-per-stage loop with mvq_rvq_rate_f32 after each search. */
int mvq_ar_latents_staged_rate_f32(const mvq_ar_args* args, int packet_tok, int min_books, int mode, float tol2, int budget,
                                   const float* z_prev, float* z_last_out, uint8_t* nb_valid_out, uint8_t* nb_sent_out, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* mvq_ar_latents_staged_rate_f32 with the search launch of each chunk replaced by mvq_rvq_beam_f32's (on the chunk's valid tokens)
 * when beam > 1; beam == 1 is that call, launch for launch; beam outside 1..8 is MVQ_EINVAL before any launch.  The rate launch
 * reads the indices as before, so z_run stays the receiver's bit for bit. */
int mvq_ar_latents_staged_rate_beam_f32(const mvq_ar_args* args, int packet_tok, int min_books, int mode, float tol2, int budget, int beam,
                                        const float* z_prev, float* z_last_out, uint8_t* nb_valid_out, uint8_t* nb_sent_out,
                                        void* workspace, size_t workspace_bytes, void* stream);
/* synchronises `stream`, then: MVQ_OK when every grid barrier of the last call on this workspace completed */
int mvq_ar_check(const void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MVQ_H */
