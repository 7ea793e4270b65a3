#!/usr/bin/env python3
"""The receiver on the MI355X: one JSON line with, per batch size B (1 / 6 / 256 one-second segments),
  * decode_latents ms  (A_QUANT.from_codes, dequantise + proj_up, the two predictor passes),
  * decode ms          (the same + T_DEC),
  * t_dec ms           (T_DEC alone on the same z_run: the "decoding delay" the reference's latency script reports),
  * pack / unpack us   (bitstream.pack_indices / unpack_indices of one item's RVQ indices and audio codes, host side).
B = 1 follows the reference's latency protocol (1 s of zeros, Evaluation/dac_vcpwq_proposed6_latency.py:517-521); B = 6 and 256
take seeded synthetic segments.  8 books x K = 512.  Timing: torch.cuda events around each call after the warm-ups, median of
the repeats; host timings with perf_counter.

  python tools/receiver_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def host_us(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    args = ap.parse_args()
    from multimodal_vqvae_compression_audio_tactile_amd import bitstream, build_proposed, synth
    dev = torch.device("cuda:0")
    books, K = 8, 512
    net = build_proposed(synth.proposed_model_state(7, rvq_books=books, rvq_embed=K), rvq_books=books, rvq_embed=K, device=dev)
    out = {"books": books, "K": K, "repeats": args.repeats, "warmup": args.warmup, "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            if B == 1:
                a = torch.zeros(1, 1, 24000, device=dev)
                t = torch.zeros(1, 1, 24000, device=dev)
            else:
                a, t = synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)
            z_tx, codes, idx = net.encode_latents_with_indices(a, t)
            z_rx = net.decode_latents(codes, idx)
            row = {"B": B,
                   "decode_latents_ms": timed(lambda: net.decode_latents(codes, idx), args.warmup, args.repeats),
                   "decode_ms": timed(lambda: net.decode(codes, idx), args.warmup, args.repeats),
                   "t_dec_ms": timed(lambda: net.T_DEC(z_rx), args.warmup, args.repeats),
                   "encode_latents_ms": timed(lambda: net.encode_latents(a, t), args.warmup, args.repeats),
                   "rx_vs_tx_rel": float((z_rx - z_tx).abs().max() / z_tx.abs().max().clamp_min(1e-30))}
            i0, c0 = idx[:, 0].cpu().numpy(), codes[0].cpu().numpy()
            pi, pa = bitstream.pack_indices(i0, K), bitstream.pack_indices(c0, 1024)
            row.update({"pack_us": host_us(lambda: (bitstream.pack_indices(i0, K), bitstream.pack_indices(c0, 1024)),
                                           args.warmup, args.repeats),
                        "unpack_us": host_us(lambda: (bitstream.unpack_indices(pi), bitstream.unpack_indices(pa)),
                                             args.warmup, args.repeats),
                        "bytes_per_item": {"tactile": len(pi), "audio": len(pa)}})
            out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
