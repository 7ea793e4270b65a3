#!/usr/bin/env python3
"""The lossy-channel receiver over the synthetic corpus of tools/corpus_eval.py (same clip lengths, seeds, native rates and
1-s segmentation; --clips of its 1 003 clips): every segment batch is sent as packets (ProposedEval.compress_packets), packets
are dropped at {0, 5, 10, 20, 50} % (plc.make_token_loss_mask at the packet size, one seeded draw per batch and rate), and the
receiver (decompress_packets) runs in each conceal mode -- "predict" (the audio-driven prediction stands in), "zero" (the
unconcealed baseline) and "plc" (an AllPredPLC predictor over the whole sequence) -- plus one row where 20 % of the packets are
not lost but THINNED to their first book.  Scores per segment against the tactile input: plc.masked_metrics (PSNR / SNR / MAE over
the lost and the kept samples, peak 1) and plc.stsim_mel_with_mask; the table holds their means over the segments (NaN-aware:
a segment without lost tokens has no masked figures).  No alignment step: the decoder's output is compared in place.

NO TRAINED CHECKPOINT EXISTS ON THESE MACHINES.  The weights are seeded random ones (synth.proposed_model_state, and a separately
seeded predictor for the PLC model), so the quality figures exercise the plumbing only -- the packet path, the three concealment
modes and the metrics -- and rank nothing: they say nothing about which mode conceals better with trained weights.

  python tools/lossy_eval.py [--clips 24] [--batch 64] [--json]
"""
import argparse
import json
import math
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

SEG = 24000
RATES = (0, 5, 10, 20, 50)
MODES = ("predict", "zero", "plc")
COLS = ("psnr_masked", "psnr_unmasked", "snr_masked", "snr_unmasked", "mae_masked", "mae_unmasked", "stsim_global", "stsim_masked",
        "stsim_unmasked")


def corpus_segments(clips, dev, mvq):
    """The segments of the first ``clips`` clips of corpus_eval.py's corpus, in its order."""
    from corpus_eval import reflect_pad_right
    up_t, up_a = mvq.Resample(3000, 24000).to(dev), mvq.Resample(44100, 24000).to(dev)
    rng = np.random.default_rng(7)
    lens24 = (rng.uniform(1.0, 4.0, 1003) * 24000 / 320).round().astype(np.int64) * 320
    gdev = torch.Generator(device=dev)
    a_segs, t_segs = [], []
    for c in range(min(clips, 1003)):
        dur = lens24[c] / 24000.0
        gdev.manual_seed(1000 + c)
        n3, n44 = int(round(dur * 3000)), int(round(dur * 44100))
        t3 = torch.cumsum(torch.randn(1, n3, generator=gdev, device=dev), -1); t3 = t3 - t3.mean(); t3 = 0.9 * t3 / t3.abs().max().clamp_min(1e-6)
        a44 = torch.randn(1, n44, generator=gdev, device=dev); a44 = 0.9 * a44 / a44.abs().max()
        t24 = up_t(t3).clamp(-1, 1)[..., :lens24[c]]
        a24 = up_a(a44).clamp(-1, 1)[..., :lens24[c]]
        L = min(t24.shape[-1], a24.shape[-1])
        nseg = int(math.ceil(lens24[c] / SEG))
        t24, a24 = reflect_pad_right(t24[..., :L], nseg * SEG - L), reflect_pad_right(a24[..., :L], nseg * SEG - L)
        for k in range(nseg):
            a_segs.append(a24[:, k * SEG:(k + 1) * SEG]); t_segs.append(t24[:, k * SEG:(k + 1) * SEG])
    return a_segs, t_segs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=24)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--books", type=int, default=8)
    ap.add_argument("--embed", type=int, default=512)
    ap.add_argument("--json", action="store_true", help="print the rows as one JSON line after the table")
    args = ap.parse_args()
    import multimodal_vqvae_compression_audio_tactile_amd as mvq
    from multimodal_vqvae_compression_audio_tactile_amd import packets, plc as P, synth
    dev = torch.device("cuda:0")
    net = mvq.build_proposed(synth.proposed_model_state(7, rvq_books=args.books, rvq_embed=args.embed),
                             rvq_books=args.books, rvq_embed=args.embed, device=dev)
    plc = mvq.AllPredPLC(net.A_ENC, net.A_QUANT, net.T_ENC, net.T_DEC, c_lat=1024)
    head = synth.proposed_head_state(23, rvq_books=1, rvq_embed=128)
    plc.predict.load_state_dict({k[len("predict."):]: v for k, v in head.items() if k.startswith("predict.")}, strict=False)
    plc = plc.to(dev).eval()
    a_segs, t_segs = corpus_segments(args.clips, dev, mvq)
    configs = [(r, m, None) for r in RATES for m in MODES] + [(20, "predict", 1)]
    acc = {c: {k: [] for k in COLS} for c in configs}
    lost_frac = {c: [] for c in configs}
    with torch.no_grad():
        for s in range(0, len(a_segs), args.batch):
            a, t = torch.stack(a_segs[s:s + args.batch]), torch.stack(t_segs[s:s + args.batch])
            B = a.shape[0]
            infos, pk, aud = net.compress_packets(a, t)
            info = infos[0]
            for rate in RATES:
                torch.manual_seed(1000 * rate + s)
                mask = P.make_token_loss_mask(B, info.T, info.packet_tok, rate / 100.0, dev)
                hit = mask.cpu().numpy()
                hit_p = [[bool(hit[b, min(q * info.packet_tok, info.T - 1)]) for q in range(info.P)] for b in range(B)]
                dropped = [[p for q, p in enumerate(pk[b]) if not hit_p[b][q]] for b in range(B)]
                thinned = [[packets.thin(p, 1, info) if hit_p[b][q] else p for q, p in enumerate(pk[b])] for b in range(B)]
                for cfg in (c for c in configs if c[0] == rate):
                    _, mode, thin_to = cfg
                    y, lost = net.decompress_packets(infos, dropped if thin_to is None else thinned, aud, conceal=mode, plc=plc)
                    assert thin_to is not None or torch.equal(lost, mask), "the receiver's lost tokens are the dropped ones"
                    assert thin_to is None or not lost.any()
                    T = min(y.shape[-1], t.shape[-1])
                    lost_frac[cfg].append(float(mask.float().mean()))
                    for b in range(B):
                        ref, est = t[b, :, :T].contiguous(), y[b, :, :T].contiguous()
                        m = P.masked_metrics(ref.reshape(-1), est.reshape(-1), mask[b], 1.0)
                        g, sm, su = P.stsim_mel_with_mask(ref, est, mask[b])
                        row = {"psnr_masked": m["psnr_masked"], "psnr_unmasked": m["psnr_unmasked"], "snr_masked": m["snr_masked"],
                               "snr_unmasked": m["snr_unmasked"], "mae_masked": m["mae_masked"], "mae_unmasked": m["mae_unmasked"],
                               "stsim_global": g, "stsim_masked": sm, "stsim_unmasked": su}
                        for k in COLS:
                            acc[cfg][k].append(row[k])
    mean = lambda v: float(np.nanmean(v)) if np.isfinite(np.asarray(v, np.float64)).any() else float("nan")
    rows = []
    for cfg in configs:
        rate, mode, thin_to = cfg
        name = f"{rate:>2d} % lost, {mode}" if thin_to is None else f"{rate:>2d} % thinned to {thin_to} book"
        rows.append({"config": name, "segments": len(acc[cfg]["stsim_global"]), "tokens_hit": float(np.mean(lost_frac[cfg])),
                     **{k: mean(acc[cfg][k]) for k in COLS}})
    print("lossy_eval: SEEDED RANDOM WEIGHTS (no trained checkpoint exists here): the figures exercise the plumbing only and rank nothing")
    print(f"{len(a_segs)} one-second segments of {args.clips} synthetic clips, {args.books} books x K = {args.embed}, "
          f"packets of {P.PACKET_TOK} tokens; 'masked' = the samples of lost (or thinned) tokens")
    print(f"{'config':<26s} {'hit':>6s} " + " ".join(f"{k:>14s}" for k in COLS))
    for r in rows:
        print(f"{r['config']:<26s} {r['tokens_hit']:>6.3f} " + " ".join(f"{r[k]:>14.4f}" for k in COLS))
    if args.json:
        print(json.dumps({"rows": rows, "note": "seeded random weights: plumbing only, ranks nothing"}))


if __name__ == "__main__":
    main()
