#!/usr/bin/env python3
"""Closed-loop sender rate control on the MI355X: one JSON line with, per batch size B (1 / 6 / 256 one-second segments,
T_lat = 75, 8 books x K = 512, packets of 2 tokens),
  (a) compress_packets_ms   the whole-item sender with rate=None, Rate(), a tol2 and a budget, and -- with --a-root, a built checkout
                            of the parent commit, in fresh child processes, --a-runs times -- the parent's compress_packets: the
                            spread of those runs is the margin within which rate=None did not move;
  (b) step_ms               the StreamSender steady step (a 16-token push onto a session fed 16 tokens at a time), eager, same rows;
  (c) rate_kernel_us        the rate kernel's own time per chunk, from the library's profile events (rvq_rate_kernel);
  (d) kbps                  the realised rate of each row, headers included and excluded (packets.sent_kbps);
  (e) drift                 per chunk index the max |z_run(sender) - z_run(receiver)| over the batch: today's OPEN loop (the sender
                            quantises with all books, the same per-packet counts applied at the receiver) next to the closed
                            loop's, which is exactly 0.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  Seeded
synthetic weights and signals: the times mean something, the rates and the drift exercise plumbing only.

  python tools/rate_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH] [--a-runs 3]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K, PTOK = 8, 512, 2
STEP = 5120


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


def inputs(B, dev, synth):
    return synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)


def steady_push(net, a, t, B, **kw):
    """A session in its steady state -> the function that pushes its next 16 tokens (the 1-s signal repeats)."""
    tx = net.stream_sender(batch=B, **kw)
    n_steps, state = a.shape[-1] // STEP, {"c": 0}

    def push():
        c = state["c"] % n_steps
        state["c"] += 1
        return tx.push(a[..., STEP * c:STEP * (c + 1)], t[..., STEP * c:STEP * (c + 1)])
    push(), push(), push()
    return push


def none_rows(args):
    """rate=None (today's path) on whatever package sys.path resolves to: (a) and (b)."""
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    rows = {}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            rows[B] = {"compress_packets_ms": timed(lambda: net.compress_packets(a, t), args.warmup, args.repeats),
                       "step_ms": timed(steady_push(net, a, t, B), args.warmup, args.repeats)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: rate=None is also measured on it, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--tol2", type=float, default=0.84)
    ap.add_argument("--budget", type=int, default=27)
    ap.add_argument("--none-only", action="store_true", help="internal: print the rate=None rows for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.none_only:
        print(json.dumps({"none": none_rows(args)}))
        return
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, ops, packets, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    parent = []
    for _ in range(args.a_runs if args.a_root else 0):
        child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--none-only", "--root", args.a_root, "--repeats",
                                str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                               capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            raise SystemExit("the parent side failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        parent.append({int(k): v for k, v in json.loads(child.stdout.strip().splitlines()[-1])["none"].items()})
    here = none_rows(args)
    rates = {"full": packets.Rate(), "tol2": packets.Rate(tol2=args.tol2), "budget": packets.Rate(budget=args.budget)}
    out = {"books": BOOKS, "K": K, "T_lat": 75, "packet_tok": PTOK, "repeats": args.repeats, "warmup": args.warmup,
           "tol2": args.tol2, "budget": args.budget, "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            row = {"B": B, "none": dict(here[B])}
            if parent:
                for key in ("compress_packets_ms", "step_ms"):
                    runs = [p[B][key] for p in parent]
                    row["none"]["parent_" + key] = {"runs": runs, "spread": max(runs) - min(runs),
                                                    "this_tree_minus_parent_median": here[B][key] - statistics.median(runs)}
            z_open, codes, idx_open = net.encode_latents_with_indices(a, t)
            info = packets.StreamInfo(K, BOOKS, idx_open.shape[2], PTOK)
            row["none"]["kbps"] = {"with_headers": packets.sent_kbps(BOOKS, info), "bodies": packets.sent_kbps(BOOKS, info, headers=False)}
            for name, rate in rates.items():
                r = {"compress_packets_ms": timed(lambda: net.compress_packets(a, t, rate=rate), args.warmup, args.repeats),
                     "step_ms": timed(steady_push(net, a, t, B, rate=rate), args.warmup, args.repeats)}
                ops.profile_begin()
                z_run, codes_r, idx, nb_sent = net.encode_latents_with_indices(a, t, rate=rate)
                prof = ops.profile_end().get("rvq_rate_kernel")
                r["rate_kernel_us"] = 1e6 * prof["seconds"] / prof["launches"]
                r["rate_kernel_launches"] = prof["launches"]
                counts = nb_sent.cpu().numpy()
                r["kbps"] = {"with_headers": statistics.mean(packets.sent_kbps(counts[b], info) for b in range(B)),
                             "bodies": statistics.mean(packets.sent_kbps(counts[b], info, headers=False) for b in range(B))}
                r["mean_books"] = float(counts.mean())
                # drift per chunk: the receiver gets these counts; the OPEN loop's sender never knew
                nb_valid = torch.repeat_interleave(nb_sent, PTOK, dim=1)[:, :info.T].contiguous()
                rx_open = net.decode_latents(codes, idx_open, nb_valid=nb_valid)
                rx_closed = net.decode_latents(codes_r, idx, nb_valid=nb_valid)
                per_chunk = lambda x, y: [float((x[..., s:s + 16] - y[..., s:s + 16]).abs().max()) for s in range(0, info.T, 16)]
                r["drift"] = {"open_loop": per_chunk(z_open, rx_open), "closed_loop": per_chunk(z_run, rx_closed)}
                row[name] = r
            out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
