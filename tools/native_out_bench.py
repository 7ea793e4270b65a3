#!/usr/bin/env python3
"""The receiver's audio output at the playback rate on the MI355X: one JSON line with
  (a) launch_ms        one steady call of the rational streamed resampler on the receiver's steady piece (16 tokens: 5120 samples at
                       24 kHz in; 9408 out at 44.1 kHz, 10240 at 48 kHz; smallest lag, the state past its start) in BOTH forms --
                       "block" (one block per session, one launch) and "split" (outputs over (parts, sessions), then the state
                       launch) -- at B = 1 / 6 / 256, the two forms alternating --runs times in this one process: per form the
                       runs, their median and their spread (max - min), and "split_faster_by_more_than_block_spread";
  (b) recv_step_ms     the StreamReceiver(audio=(1024, 32), audio_out=True, audio_fade=AudioFade(1, 4)) steady step (a 16-token push
                       onto a full history) with audio_out_rate 24000 / 44100, eager and graph=True, the two rates alternating
                       --step-runs times, and the form stream.audio_resample_form picked for that batch;
  (c) pool_round_ms    16 ticks of a StreamReceiverPoolAV(audio_out=True) in which every one of S sessions (--sessions) pushes a
                       chunk, with audio_out_rate 24000 / 44100 (one event pair around the 16 ticks).
The model, the signals, the loss pattern and the timing are tools/audio_out_bench.py's: seeded weights and signals, torch.cuda
events around each call after the warm-ups, median of the repeats; the events bracket host work too.  Only the times mean anything;
nothing is enforced.  The existing receiver rows against the parent commit are tools/stream_bench.py's and tools/audio_out_bench.py's
own --a-root runs.

  python tools/native_out_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--sessions 1,6,64] [--runs 3] [--step-runs 1]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
from audio_out_bench import AUDIO, BOOKS, K, TICKS, _net, inputs, pool_round, steady_recv, timed, timing_loss  # noqa: E402

RATES = (44100, 48000)
FORMS = ("block", "split")
PIECE = 16 * 320


def launch_rows(B, dev, args):
    """Both forms of the steady launch, alternating, per rate."""
    from multimodal_vqvae_compression_audio_tactile_amd import StreamResampleRational
    rows = {}
    for rate in RATES:
        rs = {f: StreamResampleRational(24000, rate, B, device=dev, form=f) for f in FORMS}
        x = torch.randn(B, 1, PIECE, generator=torch.Generator().manual_seed(rate)).to(dev)
        for r in rs.values():
            r.push(x[..., :1920])                                            # past the start: base = lead = 0 from here on
        runs = {f: [] for f in FORMS}
        for _ in range(args.runs):
            for f in FORMS:
                runs[f].append(timed(lambda: rs[f].push(x), args.warmup, args.repeats))
        row = {"n_in": PIECE, "n_out": rs["block"].out_len(PIECE), "state": int(rs["block"].state.shape[1])}
        for f in FORMS:
            row[f] = {"runs": runs[f], "median": statistics.median(runs[f]), "spread": max(runs[f]) - min(runs[f])}
        row["block_minus_split"] = row["block"]["median"] - row["split"]["median"]
        row["split_faster_by_more_than_block_spread"] = row["block_minus_split"] > row["block"]["spread"]
        rows[f"24000->{rate}"] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--sessions", default="1,6,64")
    ap.add_argument("--runs", type=int, default=3, help="alternations of the two forms in the launch rows")
    ap.add_argument("--step-runs", type=int, default=1, help="alternations of the two rates in the receiver and pool rows")
    args = ap.parse_args()
    from multimodal_vqvae_compression_audio_tactile_amd import stream
    from multimodal_vqvae_compression_audio_tactile_amd.packets import AudioFade
    dev = torch.device("cuda:0")
    net = _net(dev, audio_decoder=True)
    fade = AudioFade(1, 4)
    w, r = args.warmup, args.repeats
    n_push = 3 + w + r
    out = {"books": BOOKS, "K": K, "audio": list(AUDIO), "fade": [1, 4], "repeats": r, "warmup": w, "runs": args.runs,
           "step_runs": args.step_runs, "split_max": stream.AUDIO_RESAMPLE_SPLIT_MAX, "rows": [], "pool": []}
    med = lambda res: {k: {"runs": v, "median": statistics.median(v)} for k, v in res.items()}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",") if b):
            row = {"B": B, "form": stream.audio_resample_form(B), "launch_ms": launch_rows(B, dev, args)}
            if args.step_runs > 0:
                a, t = inputs(B, dev)
                infos, pk, ainfos, apk = net.compress_packets_av(a, t)
                arx = timing_loss(apk)
                res = {}
                for _ in range(args.step_runs):                              # the rates alternate: a drift of the box hits both
                    for rate in (24000, 44100):
                        kw = dict(audio_out=True, audio_fade=fade, audio_out_rate=rate)
                        for name, graph in (("eager", False), ("graph", True)):
                            res.setdefault(f"{rate}_{name}", []).append(timed(steady_recv(net, B, pk, arx, n_push, graph, **kw), w, r))
                row["recv_step_ms"] = med(res)
            out["rows"].append(row)
        for S in (int(s) for s in args.sessions.split(",") if s):
            a, t = inputs(S, dev)
            infos, pk, ainfos, apk = net.compress_packets_av(a, t)
            arx = timing_loss(apk)
            res = {}
            for _ in range(max(1, args.step_runs)):
                for rate in (24000, 44100):
                    kw = dict(audio_out=True, audio_fade=fade, audio_out_rate=rate)
                    res.setdefault(str(rate), []).append(timed(pool_round(net, S, pk, arx, **kw), 1, max(1, r // 3)))
            out["pool"].append({"sessions": S, "ticks": TICKS, "form": stream.audio_resample_form(S), "pool_round_ms": med(res)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
