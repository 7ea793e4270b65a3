"""MI355X-native encode -> vector-quantise -> decode path of Multimodal_VQVAE_compression_audio_tactile.

Drop-in surface:
  * ``DAC`` / ``Encoder`` / ``ResidualVectorQuantize`` / ``Decoder``  -- the dac.DAC(24 kHz) objects the reference
    pulls apart (``.encoder``, ``.quantizer``, ``.decoder``, ``.encode``, ``.decode``);
  * ``ResidualVQEMA`` / ``CrossPredictor`` / ``TokenNorm`` / ``PosEnc1D`` / ``AllPredAR`` / ``AllPredAR3`` (the compare_dacvsproposal_3.py
    variant) / ``ProposedEval`` / ``ProposedWrapper`` (compare_dacvsproposal_3.5_eval.py)
    -- the reference's own modules, same constructors and state-dict keys;
  * ``AllPredPLC`` / ``build_plc`` / ``make_token_loss_mask`` and the masked metrics -- packet-loss concealment (plc.py,
    PLC/PLC1.py and PLC/PLC1_eval.py), its predictor on the full-sequence attention kernels; its evaluation
    (``stsim_mel_with_mask`` / ``stsim_mel_global`` / ``mae_global`` / ``frame_token_mask`` / ``evaluate_file``);
  * ``safe_l1`` / ``MultiResSTFTLoss`` / ``MelCosineLoss`` / ``TrainingLoss`` -- the training losses (losses.py) and
    ``train`` -- the HIP-backed autograd Functions behind ``AllPredAR.forward_step(...); total.backward()``;
  * ``Resample`` / ``resample_to`` -- torchaudio.transforms.Resample as the reference calls it; ``stsim_batch``;
  * ``optim`` -- ``AdamW`` / ``clip_grad_norm_`` with torch's call shapes on HIP kernels (the reference's own
    ``torch.optim.AdamW`` works on the modules as well);
  * the receiver: ``ProposedEval.decode`` / ``decode_latents`` (z_run from the transmitted audio codes and RVQ indices),
    ``ResidualVectorQuantize.from_codes``, ``ResidualVQEMA.from_indices``, ``ProposedEval.compress`` / ``decompress`` and
    ``bitstream`` -- the byte format of the indices; over a lossy channel ``compress_packets`` / ``decompress_packets`` and
    ``decode(nb_valid=..., conceal=...)`` with ``packets`` -- the packet format (thinning, gathering what arrived); chunk by
    chunk ``ProposedEval.stream_receiver`` / ``StreamReceiver`` (``stream``: window schedule) and ``StreamResample``, for
    sessions that come and go ``ProposedEval.stream_receiver_pool`` / ``StreamReceiverPool`` (one batched step per tick), and
    the sending half ``ProposedEval.stream_sender`` / ``StreamSender`` (packets chunk by chunk, byte-equal to the whole item)
    and ``ProposedEval.stream_sender_pool`` / ``StreamSenderPool`` (sender sessions that come and go, one batched encode per tick);
    the receiver's audio output: ``ProposedEval.set_audio_decoder`` / ``build_proposed(audio_decoder=True)``, ``decode_av``,
    ``audio_out=True`` on ``decompress_packets_av`` / ``stream_receiver`` / ``StreamReceiverPoolAV`` (the audio waveform beside the
    tactile one) and ``packets.AudioFade`` (lost audio tokens fade out and back in);
  * ``ops`` -- tensor-level wrappers over the C ABI (include/mvq.h), ``synth`` -- seeded weights / signals.
All compute runs in libmvq_hip.so (hand-written HIP for gfx950); there is no CPU fallback.
"""
from . import bitstream, ops, optim, packets, stream, synth, train  # noqa: F401
from .resample import Resample, StreamResample, StreamResampleRational, resample_to  # noqa: F401
from .stream import StreamReceiver, StreamReceiverPool, StreamSender, StreamSenderNative, StreamSenderPool  # noqa: F401
from .stream import PoolChunk, StreamReceiverPoolAV, StreamSenderPoolAV  # noqa: F401
from .losses import MelCosineLoss, MultiResSTFTLoss, TrainingLoss, safe_l1, stsim_batch  # noqa: F401
from ._lib import MvqError, build, lib  # noqa: F401
from .dac import plan_overrides  # noqa: F401
from .dac import DAC, Decoder, Encoder, ResidualVectorQuantize, VectorQuantize, Snake1d, WNConv1d, WNConvTranspose1d  # noqa: F401
from .proposed import (AllPredAR, AllPredAR3, CrossPredictor, PosEnc1D, ProposedEval, ProposedWrapper, ResidualVQEMA, TokenNorm,  # noqa: F401
                       psnr_batch, psnr_global_peak_db, align_by_xcorr, crop_match, align_pair_24k,
                       psnr_3k_aligned_batch)
from .plc import (AllPredPLC, make_token_loss_mask, mae_subset, masked_metrics, psnr_subset_db, snr_subset_db,  # noqa: F401
                  token_to_sample_mask, frame_token_mask, stsim_mel_with_mask, stsim_mel_global, mae_global, evaluate_file,
                  make_category_token_loss_mask, category_mask_fn)


def build_proposed(state_dict=None, rvq_books=8, rvq_embed=512, n_codebooks=32, device="cuda", cls=None, audio_decoder=False):
    """Assemble ProposedEval exactly as the reference does (build_backbones_for_eval + ProposedEval(...),
    Evaluation/dac_vcpwq_proposed6_latency.py:527-535,660-667) and optionally load a checkpoint-shaped state dict.
    ``audio_decoder=True`` keeps the audio DAC's decoder and attaches it for the receiver's audio output
    (``net.set_audio_decoder(da.decoder)``; it is no submodule and no key of ``state_dict``: the caller loads its weights from the
    audio DAC's own checkpoint, ``net.audio_decoder.load_state_dict(...)``)."""
    da, dt = DAC(n_codebooks=n_codebooks), DAC(n_codebooks=n_codebooks)
    net = (cls or ProposedEval)(da.encoder, da.quantizer, dt.encoder, dt.decoder, c_lat=1024,
                               rvq_books=rvq_books, rvq_embed=rvq_embed)
    if state_dict is not None:
        net.load_state_dict(state_dict, strict=True)
    net = net.to(device).eval()
    if audio_decoder:
        net.set_audio_decoder(da.decoder)
    return net


def build_plc(state_dict=None, n_codebooks=32, device="cuda"):
    """Assemble AllPredPLC as the reference does (build_backbones + AllPredPLC(...), PLC/PLC1_eval.py:540-548): two DAC-24k
    instances, audio encoder / quantiser and tactile encoder / decoder, c_lat = 1024; optionally load a checkpoint's
    ``ckpt["model"]`` with strict=True."""
    da, dt = DAC(n_codebooks=n_codebooks), DAC(n_codebooks=n_codebooks)
    net = AllPredPLC(da.encoder, da.quantizer, dt.encoder, dt.decoder, c_lat=1024)
    if state_dict is not None:
        net.load_state_dict(state_dict, strict=True)
    return net.to(device).eval()
