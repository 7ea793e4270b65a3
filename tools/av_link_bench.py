#!/usr/bin/env python3
"""Audio transport on the MI355X: one JSON line with, per batch size B (1 / 6 / 256 one-second segments, T_lat = 75, 8 tactile books
x K = 512, 32 audio stages x K = 1024, packets of 2 tokens),
  (a) compress_ms / decompress_ms   compress_packets_av / decompress_packets_av with both streams whole, an audio tol2 and an audio
                                    budget, next to compress_packets / decompress_packets (the new arguments at their defaults);
  (b) audio_rate_us                 the audio rate kernels' own time per 16-token group, from the library's profile events
                                    (dac_rvq_rate_energy_kernel, dac_rvq_rate_decide_kernel, dac_rvq_from_codes_layers_kernel);
  (c) kbps                          the realised rate of both streams, headers included and excluded (packets.sent_kbps).
  (d) step_ms                       the StreamSender steady step (a 16-token push onto a session fed 16 tokens at a time, eager) with
                                    audio="packets", next to audio="codes";
  (e) recv_step_ms / recv_step_graph_ms   the StreamReceiver steady step (a 16-token push onto a session with a full history; one
                                    chunk's packets re-stamped with the sequence numbers of each push beforehand), eager and
                                    graph=True, with audio=(1024, 32) -- both streams as packets -- next to audio=None.
The existing paths (compress_packets / decompress_packets, the default sender and receiver steps) are measured in fresh child
processes, --a-runs of this tree and, with --a-root, as many of a built checkout of the parent commit: the spread of each side's
runs is the margin within which the other side did or did not move.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  Seeded
synthetic weights and signals: the times mean something, the rates exercise plumbing only.

  python tools/av_link_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH] [--a-runs 3]
"""
import argparse
import json
import struct
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K, PTOK = 8, 512, 2
STEP = 5120
KERNELS = ("dac_rvq_rate_energy_kernel", "dac_rvq_rate_decide_kernel", "dac_rvq_from_codes_layers_kernel")


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


def steady_recv(net, B, pk, audio_side, n_push, graph, audio=None):
    """A receiver session with a full history -> the function that pushes its next chunk.  ``pk``: per item the packets of a whole
    item in order; chunk 1's (sequence numbers 8..15 at 2 tokens per packet) serve every push, re-stamped beforehand.
    ``audio_side``: the chunk's audio codes [B, 32, 16] (audio None) or per item the audio packets of the whole item."""
    rx = net.stream_receiver(K, BOOKS, batch=B, graph=graph, **({"audio": audio} if audio is not None else {}))
    per = 16 // PTOK
    stamp = lambda p, seq: bytes(p[:3]) + struct.pack("<I", seq) + bytes(p[7:])
    chunk = lambda lists, c: [[stamp(p, per * c + i) for i, p in enumerate(lists[b][per:2 * per])] for b in range(B)]
    pushes = [(chunk(pk, c), audio_side if audio is None else chunk(audio_side, c)) for c in range(n_push)]
    state = {"c": 0}

    def push():
        tp, au = pushes[state["c"]]
        state["c"] += 1
        return rx.push(tp, au)
    push(), push(), push()                                               # the two shorter windows, then the steady shape (the capture)
    return push


def _net(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    return build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)


def old_rows(args):
    """The existing paths (compress_packets / decompress_packets, the default sender and receiver steps) on whatever package
    sys.path resolves to."""
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    dev = torch.device("cuda:0")
    net = _net(dev)
    rows, n_push = {}, 3 + args.warmup + args.repeats
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            sent = net.compress_packets(a, t)
            codes = net.encode_latents_with_indices(a, t)[1][..., 16:32].contiguous()
            rows[B] = {"compress_ms": timed(lambda: net.compress_packets(a, t), args.warmup, args.repeats),
                       "decompress_ms": timed(lambda: net.decompress_packets(*sent), args.warmup, args.repeats),
                       "step_ms": timed(steady_push(net, a, t, B), args.warmup, args.repeats),
                       "recv_step_ms": timed(steady_recv(net, B, sent[1], codes, n_push, False), args.warmup, args.repeats),
                       "recv_step_graph_ms": timed(steady_recv(net, B, sent[1], codes, n_push, True), args.warmup, args.repeats)}
    return rows


def children(args, root):
    """``--a-runs`` fresh child processes measuring the existing paths of the package under ``root``."""
    runs = []
    for _ in range(args.a_runs):
        child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--old-only", "--root", str(root), "--repeats",
                                str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                               capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            raise SystemExit(f"measuring {root} failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        runs.append({int(k): v for k, v in json.loads(child.stdout.strip().splitlines()[-1])["old"].items()})
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: the existing paths are also measured on it, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--audio-tol2", type=float, default=0.5)
    ap.add_argument("--audio-budget", type=int, default=100)
    ap.add_argument("--old-only", action="store_true", help="internal: print the existing paths' rows for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.old_only:
        print(json.dumps({"old": old_rows(args)}))
        return
    from multimodal_vqvae_compression_audio_tactile_amd import ops, packets, synth
    dev = torch.device("cuda:0")
    net = _net(dev)
    parent = children(args, args.a_root) if args.a_root else []
    here = children(args, ROOT)
    arates = {"full": packets.Rate(), "tol2": packets.Rate(tol2=args.audio_tol2), "budget": packets.Rate(budget=args.audio_budget)}
    out = {"books": BOOKS, "K": K, "T_lat": 75, "packet_tok": PTOK, "repeats": args.repeats, "warmup": args.warmup,
           "audio_tol2": args.audio_tol2, "audio_budget": args.audio_budget, "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            row = {"B": B, "existing": {}}
            for key in ("compress_ms", "decompress_ms", "step_ms", "recv_step_ms", "recv_step_graph_ms"):
                runs = [h[B][key] for h in here]
                e = {"runs": runs, "spread": max(runs) - min(runs)}
                if parent:
                    pr = [p[B][key] for p in parent]
                    e.update(parent_runs=pr, parent_spread=max(pr) - min(pr), median_minus_parent_median=statistics.median(runs) - statistics.median(pr))
                row["existing"][key] = e
            n_push = 3 + args.warmup + args.repeats
            for name, arate in arates.items():
                sent = net.compress_packets_av(a, t, audio_rate=arate)
                r = {"compress_ms": timed(lambda: net.compress_packets_av(a, t, audio_rate=arate), args.warmup, args.repeats),
                     "decompress_ms": timed(lambda: net.decompress_packets_av(*sent), args.warmup, args.repeats),
                     "step_ms": timed(steady_push(net, a, t, B, audio="packets", audio_rate=arate), args.warmup, args.repeats),
                     "recv_step_ms": timed(steady_recv(net, B, sent[1], sent[3], n_push, False, (1024, 32)), args.warmup, args.repeats),
                     "recv_step_graph_ms": timed(steady_recv(net, B, sent[1], sent[3], n_push, True, (1024, 32)), args.warmup, args.repeats)}
                ops.profile_begin()
                _, codes, idx, nb_sent, na_sent = net.encode_latents_with_indices(a, t, audio_rate=arate)
                prof = ops.profile_end()
                groups = B * -(-codes.shape[2] // 16)
                r["audio_rate_us"] = {k: 1e6 * prof[k]["seconds"] / prof[k]["launches"] for k in KERNELS if k in prof}
                r["audio_rate_us_per_group"] = sum(r["audio_rate_us"].values()) / groups
                info, ainfo = sent[0][0], sent[2][0]
                nbs, nas = nb_sent.cpu().numpy(), na_sent.cpu().numpy()
                mean = lambda counts, i, h: statistics.mean(packets.sent_kbps(counts[b], i, headers=h) for b in range(B))
                r["kbps"] = {"tactile": {"with_headers": mean(nbs, info, True), "bodies": mean(nbs, info, False)},
                             "audio": {"with_headers": mean(nas, ainfo, True), "bodies": mean(nas, ainfo, False)}}
                r["mean_audio_stages"] = float(nas.mean())
                row[name] = r
            out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
