#!/usr/bin/env python3
"""The streaming receiver on the MI355X: one JSON line with, per batch size B (1 / 6 / 256 sessions in lockstep, 8 books x K = 512,
packets of 2 tokens, nothing lost),
  (a) step_eager_ms / step_graph_ms   one steady push (16 new tokens, 36-token decoder window, 5120 samples out), run eagerly
                                      and as the replayed graph (StreamReceiver(graph=True)), host work included;
  (b) split                           the eager step taken apart: host gather (us), the one upload, latents (unpack +
                                      decode_latents with the carried token), window + decoder, and the 24 -> 3 kHz streamed
                                      resampler of the 5120 emitted samples (ms each, each alone);
  (c) real_time_factor                step time / 213.3 ms (the signal a chunk carries);
  (d) latency_ms                      346.7 ms (one chunk + the 10-token decoder look-ahead) + the step time;
  (e) whole_item_ms                   decompress_packets on a whole 75-token item, of this tree and -- with --a-root, a built
                                      checkout of the parent commit, in fresh child processes -- of the parent, --a-runs times:
                                      the spread of those runs is the margin within which the whole-item path did not move.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  A steady
step is timed on a session that keeps running (every timed push is a real next chunk; the packets of one chunk are re-numbered on
the host for each).  Seeded synthetic weights and signals: only the times mean anything.

  python tools/stream_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH] [--a-runs 3]
"""
import argparse
import json
import statistics
import struct
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K, T_ITEM = 8, 512, 75
CHUNK_MS, LOOKAHEAD_MS = 16 / 75 * 1000.0, 10 / 75 * 1000.0


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
    return synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)


def whole_item_rows(args):
    """(e) on whatever package sys.path resolves to."""
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    rows = {}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            infos, pk, aud = net.compress_packets(a, t)
            rows[B] = timed(lambda: net.decompress_packets(infos, pk, aud), args.warmup, args.repeats)
    return rows


def renumber(pkt, seq):
    """The same packet under another sequence number (the header's uint32 at offset 3)."""
    return pkt[:3] + struct.pack("<I", seq) + pkt[7:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: (e) is also measured on it, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--whole-only", action="store_true", help="internal: print (e) for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.whole_only:
        print(json.dumps({"whole": whole_item_rows(args)}))
        return
    from multimodal_vqvae_compression_audio_tactile_amd import StreamResample, bitstream, build_proposed, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    parent = []
    for _ in range(args.a_runs if args.a_root else 0):
        child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--whole-only", "--root", args.a_root, "--repeats",
                                str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                               capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            raise SystemExit("the parent side failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        parent.append({int(k): v for k, v in json.loads(child.stdout.strip().splitlines()[-1])["whole"].items()})
    here = whole_item_rows(args)
    out = {"books": BOOKS, "K": K, "packet_tok": 2, "chunk_tok": 16, "window_tok": 36, "repeats": args.repeats, "warmup": args.warmup,
           "chunk_ms": CHUNK_MS, "lookahead_ms": LOOKAHEAD_MS, "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            infos, pk, aud = net.compress_packets(a, t)
            codes = torch.from_numpy(np.stack([bitstream.unpack_indices(p)[0] for p in aud]))[..., 16:32].contiguous()
            chunk1 = [item[8:16] for item in pk]                              # the packets of tokens 16..31

            def session(graph):
                rx = net.stream_receiver(K, BOOKS, batch=B, graph=graph)
                state = {"c": 0}

                def push():
                    c = state["c"]
                    state["c"] += 1
                    return rx.push([[renumber(p, 8 * c + j) for j, p in enumerate(item)] for item in chunk1], codes)
                push(), push()                                                # the two warming-up shapes (16, 32 tokens)
                return rx, push

            row = {"B": B}
            for name, graph in (("step_eager_ms", False), ("step_graph_ms", True)):
                _, push = session(graph)
                row[name] = timed(push, args.warmup, args.repeats)
            # the eager step's stages, each alone, on a session in its steady state
            rx, push = session(False)
            push()
            numbered = [[renumber(p, rx.tokens // 2 + j) for j, p in enumerate(item)] for item in chunk1]
            late0 = rx.late
            host = rx._gather(numbered, 16)
            assert rx.late == late0
            up, codes_d = torch.from_numpy(host).to(dev), codes.to(dev)
            plan = rx._plan(16, False)
            assert plan == (20, 20, 3200, 8320)
            z = rx._latents(up, codes_d, 16)
            y = rx._window_decode(z, *plan)
            rs = StreamResample(24000, 3000, B, device=dev)
            rs.push(y), rs.push(y)

            def upload():
                torch.from_numpy(host).to(dev), codes.to(dev)
            row["split"] = {"host_gather_us": host_us(lambda: rx._gather(numbered, 16), args.warmup, args.repeats),
                            "upload_ms": timed(upload, args.warmup, args.repeats),
                            "latents_ms": timed(lambda: rx._latents(up, codes_d, 16), args.warmup, args.repeats),
                            "window_decoder_ms": timed(lambda: rx._window_decode(z, *plan), args.warmup, args.repeats),
                            "resample_ms": timed(lambda: rs.push(y), args.warmup, args.repeats)}
            for name in ("step_eager_ms", "step_graph_ms"):
                row[name.replace("_ms", "_real_time_factor")] = row[name] / CHUNK_MS
                row[name.replace("step_", "latency_")] = CHUNK_MS + LOOKAHEAD_MS + row[name]
            row["whole_item_ms"] = {"this_tree": here[B], "parent_runs": [p[B] for p in parent]}
            if parent:
                runs = row["whole_item_ms"]["parent_runs"]
                row["whole_item_ms"]["parent_spread"] = max(runs) - min(runs)
                row["whole_item_ms"]["this_tree_minus_parent_median"] = here[B] - statistics.median(runs)
            out["rows"].append(row)
    print(json.dumps(out))
    if any(r["B"] == 1 and min(r["step_eager_ms"], r["step_graph_ms"]) >= CHUNK_MS for r in out["rows"]):
        raise SystemExit("one session does not keep up with real time: the B = 1 step takes longer than the 213.3 ms chunk it decodes")


if __name__ == "__main__":
    main()
