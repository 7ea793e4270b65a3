#!/usr/bin/env python3
"""The lossy-channel receiver on the MI355X: one JSON line with, per batch size B (1 / 6 / 256 one-second segments, T_lat = 75,
8 books x K = 512, packets of 2 tokens),
  (a) decompress_v1_ms        ProposedEval.decompress on v1 payloads (bitstream.py) -- of the tree named by --a-root (a checkout of
                              the parent commit, built; measured in a fresh child process) or, without it, of this tree;
  (b) packets_0pct_ms         decompress_packets with every packet delivered;
  (c) packets_20pct_ms        decompress_packets at 20 % packet loss, per conceal mode ("predict", "zero", "plc");
  (d) split_0pct              (b) taken apart: host gather (us), the one upload, the device unpack and decode (ms each); the audio
                              side's v1 unpack + upload, which both paths share, is reported next to them.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats -- the events bracket host work too (the
stream is idle when the first is recorded), so (a)-(c) are wall-clock figures of one call; host-only pieces use perf_counter.
Seeded synthetic weights and signals: no trained checkpoint exists here, so only the times mean anything.

  python tools/lossy_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K = 8, 512


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


def inputs(B, dev, synth):
    if B == 1:                                                        # the reference's latency protocol: 1 s of zeros
        return torch.zeros(1, 1, 24000, device=dev), torch.zeros(1, 1, 24000, device=dev)
    return synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)


def v1_rows(args):
    """(a) on whatever package sys.path resolves to."""
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    rows = {}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            tac, aud = net.compress(a, t)
            rows[B] = timed(lambda: net.decompress(tac, aud), args.warmup, args.repeats)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: (a) is measured on it, in a child process")
    ap.add_argument("--v1-only", action="store_true", help="internal: print (a) for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.v1_only:
        print(json.dumps({"v1": v1_rows(args)}))
        return
    from multimodal_vqvae_compression_audio_tactile_amd import bitstream, build_proposed, ops, packets, plc as plc_mod, synth
    from multimodal_vqvae_compression_audio_tactile_amd import AllPredPLC
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    plc = AllPredPLC(net.A_ENC, net.A_QUANT, net.T_ENC, net.T_DEC, c_lat=1024)
    head = synth.proposed_head_state(23, rvq_books=1, rvq_embed=128)
    plc.predict.load_state_dict({k[len("predict."):]: v for k, v in head.items() if k.startswith("predict.")}, strict=False)
    plc = plc.to(dev).eval()
    if args.a_root:
        child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--v1-only", "--root", args.a_root, "--repeats",
                                str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                               capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            raise SystemExit("the A side failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        a_side = {int(k): v for k, v in json.loads(child.stdout.strip().splitlines()[-1])["v1"].items()}
        a_what = "parent checkout (child process)"
    else:
        a_side, a_what = v1_rows(args), "this tree (decompress and its kernels are unchanged by the packet path)"
    out = {"books": BOOKS, "K": K, "T_lat": 75, "packet_tok": plc_mod.PACKET_TOK, "repeats": args.repeats, "warmup": args.warmup,
           "a_side": a_what, "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            infos, pk, aud = net.compress_packets(a, t)
            info = infos[0]
            torch.manual_seed(20 + B)
            lost = plc_mod.make_token_loss_mask(B, info.T, info.packet_tok, 0.2, dev).cpu().numpy()
            rx = [[p for s, p in enumerate(pk[b]) if not lost[b, min(s * info.packet_tok, info.T - 1)]] for b in range(B)]
            row = {"B": B, "decompress_v1_ms": a_side[B],
                   "packets_0pct_ms": timed(lambda: net.decompress_packets(infos, pk, aud), args.warmup, args.repeats),
                   "packets_20pct_ms": {c: timed(lambda: net.decompress_packets(infos, rx, aud, conceal=c, plc=plc),
                                                 args.warmup, args.repeats) for c in ("predict", "zero", "plc")},
                   "tokens_lost_20pct": float(lost.mean())}
            row["packets_0pct_over_v1"] = row["packets_0pct_ms"] / row["decompress_v1_ms"]
            # (d) the pieces of (b), each alone
            P, full = info.P, packets.body_bytes(info.packet_tok, info.nb, info.K)
            gathered = [packets.gather(pk[b], info) for b in range(B)]
            host = np.concatenate([np.stack([g[0] for g in gathered]).reshape(-1), np.stack([g[1] for g in gathered]).reshape(-1)])
            up = torch.from_numpy(host).to(dev)
            bod, rcv = up[:B * P * full].view(B, P, full), up[B * P * full:].view(B, P)
            idx, nbv = ops.idx_unpack_packets(bod, rcv, info.K, info.nb, info.T, info.packet_tok)
            codes = torch.from_numpy(np.stack([bitstream.unpack_indices(p)[0] for p in aud])).to(dev)
            row["split_0pct"] = {
                "host_gather_us": host_us(lambda: [packets.gather(pk[b], info) for b in range(B)], args.warmup, args.repeats),
                "upload_ms": timed(lambda: torch.from_numpy(host).to(dev), args.warmup, args.repeats),
                "device_unpack_ms": timed(lambda: ops.idx_unpack_packets(bod, rcv, info.K, info.nb, info.T, info.packet_tok),
                                          args.warmup, args.repeats),
                "decode_ms": timed(lambda: net.decode(codes, idx, nb_valid=nbv), args.warmup, args.repeats),
                "audio_v1_unpack_upload_us": host_us(
                    lambda: torch.from_numpy(np.stack([bitstream.unpack_indices(p)[0] for p in aud])).to(dev), args.warmup, args.repeats)}
            tac_v1 = net.compress(a, t)[0]
            row["split_0pct"]["v1_tactile_unpack_us"] = host_us(lambda: [bitstream.unpack_indices(p) for p in tac_v1],
                                                                args.warmup, args.repeats)
            row["bytes_per_item"] = {"packets": sum(len(p) for p in pk[0]), "v1": len(tac_v1[0])}
            out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
