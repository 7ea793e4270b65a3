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
                                      With --a-root the two trees ALTERNATE (parent, this tree, parent, ...), each child also
                                      times the default steady step (eager and graph): default_step holds both trees' runs;
  (f) stateful                        with --decoder stateful: the same session with StreamReceiver(decoder="stateful") (DESIGN.md
                                      section 23) in the same run -- its steady step, eager and replayed, and its decode stage
                                      (stage windows + T_DEC piece) next to the window mode's "window + decoder" stage, both
                                      with minimum and maximum over the repeats, their ratio, and the state bytes per session.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  A steady
step is timed on a session that keeps running (every timed push is a real next chunk; the packets of one chunk are re-numbered on
the host for each).  Seeded synthetic weights and signals: only the times mean anything.

  python tools/stream_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH] [--a-runs 3] [--decoder window|stateful]
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


def timed_all(fn, warmup, repeats):
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
    return ms


def timed(fn, warmup, repeats):
    return statistics.median(timed_all(fn, warmup, repeats))


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def host_us(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    us = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        us.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(us)


def renumber(pkt, seq):
    """The same packet under another sequence number (the header's uint32 at offset 3)."""
    return pkt[:3] + struct.pack("<I", seq) + pkt[7:]


def inputs(B, dev, synth):
    return synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)


def steady_session(net, B, chunk1, codes, graph, **kw):
    """A StreamReceiver past its two warming-up shapes (16, 32 tokens) -> (session, push): every push is a real next chunk."""
    rx = net.stream_receiver(K, BOOKS, batch=B, graph=graph, **kw)
    state = {"c": 0}

    def push():
        c = state["c"]
        state["c"] += 1
        return rx.push([[renumber(p, 8 * c + j) for j, p in enumerate(item)] for item in chunk1], codes)
    push(), push()
    return rx, push


def whole_item_rows(args):
    """(e) on whatever package sys.path resolves to: decompress_packets, and the default steady step (no decoder= argument: the
    parent commit has none)."""
    from multimodal_vqvae_compression_audio_tactile_amd import bitstream, build_proposed, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    rows, steps = {}, {}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            infos, pk, aud = net.compress_packets(a, t)
            rows[B] = timed(lambda: net.decompress_packets(infos, pk, aud), args.warmup, args.repeats)
            codes = torch.from_numpy(np.stack([bitstream.unpack_indices(p)[0] for p in aud]))[..., 16:32].contiguous()
            chunk1 = [item[8:16] for item in pk]
            steps[B] = {name: timed(steady_session(net, B, chunk1, codes, graph)[1], args.warmup, args.repeats)
                        for name, graph in (("step_eager_ms", False), ("step_graph_ms", True))}
    return rows, steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: (e) is also measured on it, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--whole-only", action="store_true", help="internal: print (e) for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    ap.add_argument("--decoder", choices=("window", "stateful"), default="window",
                    help="stateful: also measure StreamReceiver(decoder='stateful') in the same run (f)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.whole_only:
        whole, steps = whole_item_rows(args)
        print(json.dumps({"whole": whole, "steps": steps}))
        return
    from multimodal_vqvae_compression_audio_tactile_amd import StreamResample, bitstream, build_proposed, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    parent, parent_steps, mine, mine_steps = [], [], [], []

    def child_run(root):
        child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--whole-only", "--root", root, "--repeats",
                                str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                               capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            raise SystemExit(f"the child on {root} failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        print(f"stream_bench: child on {root} done", file=sys.stderr, flush=True)
        got = json.loads(child.stdout.strip().splitlines()[-1])
        return {int(k): v for k, v in got["whole"].items()}, {int(k): v for k, v in got["steps"].items()}

    for _ in range(args.a_runs if args.a_root else 0):                        # the two trees alternate, each in fresh processes
        for root, whole, steps in ((args.a_root, parent, parent_steps), (args.root, mine, mine_steps)):
            w, st = child_run(root)
            whole.append(w), steps.append(st)
    here = whole_item_rows(args)[0]
    out = {"books": BOOKS, "K": K, "packet_tok": 2, "chunk_tok": 16, "window_tok": 36, "repeats": args.repeats, "warmup": args.warmup,
           "chunk_ms": CHUNK_MS, "lookahead_ms": LOOKAHEAD_MS, "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            infos, pk, aud = net.compress_packets(a, t)
            codes = torch.from_numpy(np.stack([bitstream.unpack_indices(p)[0] for p in aud]))[..., 16:32].contiguous()
            chunk1 = [item[8:16] for item in pk]                              # the packets of tokens 16..31

            def session(graph, **kw):
                return steady_session(net, B, chunk1, codes, graph, **kw)

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
            win_dec = timed_all(lambda: rx._window_decode(z, *plan), args.warmup, args.repeats)
            row["split"] = {"host_gather_us": host_us(lambda: rx._gather(numbered, 16), args.warmup, args.repeats),
                            "upload_ms": timed(upload, args.warmup, args.repeats),
                            "latents_ms": timed(lambda: rx._latents(up, codes_d, 16), args.warmup, args.repeats),
                            "window_decoder_ms": statistics.median(win_dec),
                            "resample_ms": timed(lambda: rs.push(y), args.warmup, args.repeats)}
            if args.decoder == "stateful":                                    # (f): the same session on the stateful decoder
                sf = {name: timed(session(graph, decoder="stateful")[1], args.warmup, args.repeats)
                      for name, graph in (("step_eager_ms", False), ("step_graph_ms", True))}
                rxs, pushs = session(False, decoder="stateful")
                pushs()
                ys = rxs._window_decode(z, *plan)                             # a steady step leaves the state in the steady shape
                assert ys.shape == y.shape
                sf_dec = timed_all(lambda: rxs._window_decode(z, *plan), args.warmup, args.repeats)
                sf["decode_stage_ms"], sf["window_mode_decode_stage_ms"] = spread(sf_dec), spread(win_dec)
                sf["decode_stage_ratio"] = statistics.median(win_dec) / statistics.median(sf_dec)
                sf["faster_by_more_than_window_spread"] = bool(
                    statistics.median(win_dec) - statistics.median(sf_dec) > max(win_dec) - min(win_dec))
                sf["state_bytes_per_session"] = 4 * rxs.dec_state.shape[1]
                sf["window_mode_state_bytes_per_session"] = 4 * rx.hist.shape[1] * rx.hist.shape[2]
                row["stateful"] = sf
            for name in ("step_eager_ms", "step_graph_ms"):
                row[name.replace("_ms", "_real_time_factor")] = row[name] / CHUNK_MS
                row[name.replace("step_", "latency_")] = CHUNK_MS + LOOKAHEAD_MS + row[name]
            row["whole_item_ms"] = {"this_tree": here[B], "parent_runs": [p[B] for p in parent]}
            if parent:
                runs = row["whole_item_ms"]["parent_runs"]
                row["whole_item_ms"]["this_tree_runs"] = [m[B] for m in mine]
                row["whole_item_ms"]["parent_spread"] = max(runs) - min(runs)
                row["whole_item_ms"]["this_tree_minus_parent_median"] = statistics.median(m[B] for m in mine) - statistics.median(runs)
                row["default_step"] = {}
                for name in ("step_eager_ms", "step_graph_ms"):
                    pr, mr = [p[B][name] for p in parent_steps], [m[B][name] for m in mine_steps]
                    row["default_step"][name] = {"parent_runs": pr, "this_tree_runs": mr, "parent_spread": max(pr) - min(pr),
                                                 "this_tree_minus_parent_median": statistics.median(mr) - statistics.median(pr)}
            out["rows"].append(row)
    print(json.dumps(out))
    if any(r["B"] == 1 and min(r["step_eager_ms"], r["step_graph_ms"]) >= CHUNK_MS for r in out["rows"]):
        raise SystemExit("one session does not keep up with real time: the B = 1 step takes longer than the 213.3 ms chunk it decodes")


if __name__ == "__main__":
    main()
