#!/usr/bin/env python3
"""The native-rate sender on the MI355X: one JSON line with, per batch size B (1 / 6 / 256 sessions in lockstep),
  (a) resample_ms      one steady launch of the rational streamed resampler (mvq_resample_stream_rational_f32) on 16 tokens of
                       input, for 44100 -> 24000 (hold 4), 3000 -> 24000 (hold 40) and 24000 -> 44100 (hold 4): the state is past
                       its start, so every timed call is the same launch on the next samples;
  (b) native_step_*    StreamSenderNative's steady push (16 tokens of 44.1 kHz audio and 3 kHz tactile samples: two resample
                       launches, then the inner session's steady step), eagerly and with graph=True, host work included;
  (c) inner_step_*     beside each, the inner StreamSender's steady step on 24 kHz samples, measured in the same run; the difference
                       is what the front end costs;
  (d) with --a-root    (a built checkout of the parent commit) the rows of tools/stream_send_bench.py against the parent, both
                       trees alternating in that tool's one call: "existing_path" holds its JSON line as it is.  No code on that
                       path changed; a row outside the parent's own run-to-run spread is listed under "outside_parent_spread".
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  Seeded
synthetic weights and signals: only the times mean anything.  Nothing is enforced.

  python tools/native_rate_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH] [--a-runs 3]
"""
import argparse
import json
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from stream_send_bench import BOOKS, K, STEP, steady_session, timed  # noqa: E402

RATIOS = ((44100, 24000, 4), (3000, 24000, 40), (24000, 44100, 4))           # (in Hz, out Hz, hold = the blocks of one token)
TOK = 16


def resample_rows(B, dev, args):
    from multimodal_vqvae_compression_audio_tactile_amd import StreamResampleRational
    rows = {}
    for fi, fo, hold in RATIOS:
        rs = StreamResampleRational(fi, fo, B, device=dev, hold=hold)
        n = TOK * hold * rs.orig
        x = torch.randn(B, 1, n, generator=torch.Generator().manual_seed(fi)).to(dev)
        rs.push(x)                                                             # past the start: base = lead = 0 from here on
        rows[f"{fi}->{fo}"] = {"n_in": n, "n_out": rs.out_len(n), "state": int(rs.state.shape[1]),
                               "ms": timed(lambda: rs.push(x), args.warmup, args.repeats)}
    return rows


def native_session(net, a, t, B, graph):
    """A StreamSenderNative in its steady state -> push: three 16-token pushes have run (15 tokens, chunk 0, the first steady step)."""
    tx = net.stream_sender_native(batch=B, graph=graph)
    ta, tt = tx.samples_per_token
    n_steps = min(a.shape[-1] // (TOK * ta), t.shape[-1] // (TOK * tt))
    state = {"c": 0}

    def push():
        c = state["c"] % n_steps
        state["c"] += 1
        return tx.push(a[..., TOK * ta * c:TOK * ta * (c + 1)], t[..., TOK * tt * c:TOK * tt * (c + 1)])
    push(), push(), push()
    return push


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: tools/stream_send_bench.py runs against it")
    ap.add_argument("--a-runs", type=int, default=3)
    args = ap.parse_args()
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    out = {"books": BOOKS, "K": K, "tokens_per_push": TOK, "repeats": args.repeats, "warmup": args.warmup, "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            row = {"B": B, "resample_ms": resample_rows(B, dev, args)}
            a24, t24 = synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)
            a, t = synth.audio_segments(B, seed=11, T=44100, sr=44100).to(dev), synth.tactile_segments(B, seed=11, T=3000, sr=3000).to(dev)
            assert STEP == TOK * 320
            for name, graph in (("eager", False), ("graph", True)):
                row[f"native_step_{name}_ms"] = timed(native_session(net, a, t, B, graph), args.warmup, args.repeats)
                row[f"inner_step_{name}_ms"] = timed(steady_session(net, a24, t24, B, graph)[1], args.warmup, args.repeats)
                row[f"front_end_{name}_ms"] = row[f"native_step_{name}_ms"] - row[f"inner_step_{name}_ms"]
            out["rows"].append(row)
    if args.a_root:
        child = subprocess.run([sys.executable, str(ROOT / "tools" / "stream_send_bench.py"), "--a-root", args.a_root, "--a-runs",
                                str(args.a_runs), "--repeats", str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                               capture_output=True, text=True, timeout=1500)
        if child.returncode != 0:
            raise SystemExit("tools/stream_send_bench.py failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        old = json.loads(child.stdout.strip().splitlines()[-1])
        out["existing_path"] = old
        outside = []
        for r in old["rows"]:
            for what, here_runs, parent_runs in (("whole_item_ms", r["whole_item_ms"]["this_tree_runs"], r["whole_item_ms"]["parent_runs"]),
                                                 ("window_step_eager_ms", *[[x[0] for x in r["window_step_ms"][k]] for k in ("this_tree_runs", "parent_runs")]),
                                                 ("window_step_graph_ms", *[[x[1] for x in r["window_step_ms"][k]] for k in ("this_tree_runs", "parent_runs")])):
                lo, hi = min(parent_runs), max(parent_runs)
                for v in here_runs:
                    if not lo <= v <= hi:
                        outside.append({"B": r["B"], "row": what, "this_tree": v, "parent_min": lo, "parent_max": hi})
        out["outside_parent_spread"] = outside
    print(json.dumps(out))


if __name__ == "__main__":
    main()
