#!/usr/bin/env python3
"""Receiver-side audio concealment on the MI355X: one JSON line with
  (a) times, per batch size B (1 / 6 / 256 one-second segments, T_lat = 75, 8 tactile books x K = 512, 32 audio stages x K = 1024,
      packets of 2 tokens; every other audio packet of chunk 1 and one packet of every other chunk lost):
        decode_latents_ms / decompress_av_ms   decode_latents(na_valid=) and decompress_packets_av under audio_conceal = "zero" /
                                               "mask" / "hold";
        recv_step_ms / recv_step_graph_ms      the StreamReceiver(audio=(1024, 32)) steady step (a 16-token push onto a session with a
                                               full history), eager and graph=True, under the three modes, at B = 1 and 256;
      each --a-runs times, the three modes alternating;
      the EXISTING paths -- decode_latents with na_valid=None and with na_valid (no audio_conceal argument), decompress_packets,
      decompress_packets_av, the default and the audio=(1024, 32) receiver steps -- are measured in fresh child processes, --a-runs of
      this tree and, with --a-root, as many of a built checkout of the parent commit, ALTERNATING the two trees: the spread of the
      parent's runs is the margin within which this tree did or did not move;
  (b) per-chunk drift: ||z_run - z_run_lossless|| over each 16-token chunk, relative to ||z_run_lossless|| of that chunk, mean over the
      chunks that lost at least one audio token, under the three modes, over a seeded channel that drops 5 / 10 / 20 % of the audio
      packets (the tactile stream whole).  Seeded synthetic weights: this shows the plumbing, it says nothing about quality.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.

  python tools/audio_conceal_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH] [--a-runs 3]
"""
import argparse
import json
import statistics
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K, PTOK, AUDIO = 8, 512, 2, (1024, 32)
MODES = ("zero", "mask", "hold")
STREAM_B = (1, 256)


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


def _net(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    return build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)


def inputs(B, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    return synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)


def timing_loss(apk):
    """The audio packets that arrive in the timed runs: per item every other packet of chunk 1 and packet 8c + 3 of every other
    chunk are lost."""
    drop = lambda s: (8 <= s < 16 and s % 2 == 1) or (not 8 <= s < 16 and s % 8 == 3)
    return [[p for s, p in enumerate(lst) if not drop(s)] for lst in apk]


def steady_recv(net, B, pk, audio_side, n_push, graph, **kw):
    """A receiver session with a full history -> the function that pushes its next chunk.  ``pk`` / ``audio_side``: per item the
    packets of chunk 1 that arrive (sequence numbers 8..15); they serve every push, re-stamped beforehand.  ``audio_side`` may be
    the chunk's audio codes [B, 32, 16] instead (sessions without audio=)."""
    rx = net.stream_receiver(K, BOOKS, batch=B, graph=graph, **kw)
    per = 16 // PTOK
    seq = lambda p: int.from_bytes(bytes(p)[3:7], "little")
    stamp = lambda p, c: bytes(p[:3]) + struct.pack("<I", per * c + seq(p) - per) + bytes(p[7:])
    chunk = lambda lists, c: [[stamp(p, c) for p in lists[b] if per <= seq(p) < 2 * per] for b in range(B)]
    pushes = [(chunk(pk, c), chunk(audio_side, c) if isinstance(audio_side, list) else audio_side) for c in range(n_push)]
    state = {"c": 0}

    def push():
        tp, au = pushes[state["c"]]
        state["c"] += 1
        return rx.push(tp, au)
    push(), push(), push()                                               # the two shorter windows, then the steady shape (the capture)
    return push


def old_rows(args):
    """The existing paths on whatever package sys.path resolves to (no audio_conceal argument anywhere)."""
    dev = torch.device("cuda:0")
    net = _net(dev)
    rows, n_push = {}, 3 + args.warmup + args.repeats
    w, r = args.warmup, args.repeats
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev)
            sent = net.compress_packets(a, t)
            infos, pk, ainfos, apk = net.compress_packets_av(a, t)
            arx = timing_loss(apk)
            _, codes, idx = net.encode_latents_with_indices(a, t)
            nav = torch.full((B, codes.shape[2]), 32, dtype=torch.uint8, device=dev)
            nav[:, 17:32:4] = 0
            nav[:, 18:32:4] = 0
            row = {"decode_latents_ms": timed(lambda: net.decode_latents(codes, idx), w, r),
                   "decode_latents_na_ms": timed(lambda: net.decode_latents(codes, idx, na_valid=nav), w, r),
                   "decompress_ms": timed(lambda: net.decompress_packets(*sent), w, r),
                   "decompress_av_ms": timed(lambda: net.decompress_packets_av(infos, pk, ainfos, arx), w, r)}
            if B in STREAM_B:
                c16 = codes[..., 16:32].contiguous()
                row.update(recv_step_ms=timed(steady_recv(net, B, sent[1], c16, n_push, False), w, r),
                           recv_step_graph_ms=timed(steady_recv(net, B, sent[1], c16, n_push, True), w, r),
                           recv_step_av_ms=timed(steady_recv(net, B, pk, arx, n_push, False, audio=AUDIO), w, r),
                           recv_step_av_graph_ms=timed(steady_recv(net, B, pk, arx, n_push, True, audio=AUDIO), w, r))
            rows[B] = row
    return rows


def child(args, root):
    """One fresh child process measuring the existing paths of the package under ``root``."""
    c = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--old-only", "--root", str(root), "--repeats",
                        str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                       capture_output=True, text=True, timeout=900)
    if c.returncode != 0:
        raise SystemExit(f"measuring {root} failed:\n" + c.stdout[-2000:] + c.stderr[-2000:])
    return {int(k): v for k, v in json.loads(c.stdout.strip().splitlines()[-1])["old"].items()}


def drift(net, dev, B, losses, seed):
    """(b): per loss rate and mode the mean over the affected chunks of ||z_run - z_lossless|| / ||z_lossless||, chunk by chunk."""
    a, t = inputs(B, dev)
    _, codes, idx = net.encode_latents_with_indices(a, t)
    T = codes.shape[2]
    z0 = net.decode_latents(codes, idx)
    r = np.random.default_rng(seed)
    out = {}
    for loss in losses:
        P = -(-T // PTOK)
        got = r.uniform(size=(B, P)) >= loss                                  # packets that arrive
        nav = torch.from_numpy(np.repeat(got, PTOK, axis=1)[:, :T].astype(np.uint8) * 32).to(dev)
        nc = -(-T // 16)
        hit = torch.stack([(nav[:, 16 * c:16 * c + 16] == 0).any(dim=1) for c in range(nc)], dim=1)      # [B, chunks]
        row = {"lost_tokens": float((nav == 0).float().mean()), "chunks_hit": int(hit.sum())}
        for mode in MODES:
            z = net.decode_latents(codes, idx, na_valid=nav, audio_conceal=mode)
            num = torch.stack([(z - z0)[:, :, 16 * c:16 * c + 16].flatten(1).norm(dim=1) for c in range(nc)], dim=1)
            den = torch.stack([z0[:, :, 16 * c:16 * c + 16].flatten(1).norm(dim=1) for c in range(nc)], dim=1)
            rel = (num / den)[hit]
            row[mode] = float(rel.mean()) if rel.numel() else 0.0
        out[f"{int(round(100 * loss))}%"] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: the existing paths are also measured on it, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--drift-batch", type=int, default=64)
    ap.add_argument("--old-only", action="store_true", help="internal: print the existing paths' rows for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.old_only:
        print(json.dumps({"old": old_rows(args)}))
        return
    parent, here = [], []
    for _ in range(args.a_runs):                                             # the two trees alternate
        if args.a_root:
            parent.append(child(args, args.a_root))
        here.append(child(args, ROOT))
    dev = torch.device("cuda:0")
    net = _net(dev)
    out = {"books": BOOKS, "K": K, "T_lat": 75, "packet_tok": PTOK, "repeats": args.repeats, "warmup": args.warmup, "rows": []}
    w, r = args.warmup, args.repeats
    n_push = 3 + w + r
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev)
            row = {"B": B, "existing": {}}
            for key in here[0][B]:
                runs = [h[B][key] for h in here]
                e = {"runs": runs, "spread": max(runs) - min(runs)}
                if parent:
                    pr = [p[B][key] for p in parent]
                    e.update(parent_runs=pr, parent_spread=max(pr) - min(pr),
                             median_minus_parent_median=statistics.median(runs) - statistics.median(pr))
                    e["inside_parent_spread"] = abs(e["median_minus_parent_median"]) <= e["parent_spread"]
                row["existing"][key] = e
            infos, pk, ainfos, apk = net.compress_packets_av(a, t)
            arx = timing_loss(apk)
            _, codes, idx = net.encode_latents_with_indices(a, t)
            nav = torch.full((B, codes.shape[2]), 32, dtype=torch.uint8, device=dev)
            nav[:, 17:32:4] = 0
            nav[:, 18:32:4] = 0
            res = {mode: {} for mode in MODES}
            for _ in range(args.a_runs):                                     # the modes alternate too: a drift of the box hits all three
                for mode in MODES:
                    m = {"decode_latents_ms": timed(lambda: net.decode_latents(codes, idx, na_valid=nav, audio_conceal=mode), w, r),
                         "decompress_av_ms": timed(lambda: net.decompress_packets_av(infos, pk, ainfos, arx, audio_conceal=mode), w, r)}
                    if B in STREAM_B:
                        kw = dict(audio=AUDIO, audio_conceal=mode)
                        m.update(recv_step_ms=timed(steady_recv(net, B, pk, arx, n_push, False, **kw), w, r),
                                 recv_step_graph_ms=timed(steady_recv(net, B, pk, arx, n_push, True, **kw), w, r))
                    for k, v in m.items():
                        res[mode].setdefault(k, []).append(v)
            for mode in MODES:
                row[mode] = {k: {"runs": v, "median": statistics.median(v)} for k, v in res[mode].items()}
            out["rows"].append(row)
        out["drift"] = {"B": args.drift_batch, "note": "seeded weights: plumbing only, no statement about quality",
                        "relative_l2_per_hit_chunk": drift(net, dev, args.drift_batch, (0.05, 0.10, 0.20), seed=3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
