#!/usr/bin/env python3
"""The receiver pool on the MI355X: one JSON line with, per number of sessions S (1 / 6 / 64 / 256; 8 books
x K = 512, packets of 2 tokens, nothing lost), all in this one process,
  (a) tick_ms          one StreamReceiverPool.step, host work included.  Session i starts (i mod 16) token-times late and one tick
                       per token-time (13.3 ms of signal) serves the sessions whose 16-token chunk completed with it: the
                       sessions with i mod 16 == tick mod 16, about S/16 of them, all in the steady group once each has three
                       chunks behind it.  Median, minimum and maximum over the timed ticks that served a session (with S < 16
                       the others serve none and return at once; they are timed too and counted in (b));
  (b) round_ms         the sum of 16 consecutive ticks: every one of the S sessions advanced by one chunk, 213.3 ms of signal.
                       Median, minimum and maximum over the timed rounds.  THE THRESHOLD: the median must stay under 213.3 ms;
  (c) lockstep_ms      one steady eager StreamReceiver(batch=S).push -- the same S chunks as ONE batch, which needs the S sessions
                       in lockstep; and round_over_lockstep = (b) / (c), what serving them out of step costs;
  (d) solo_ms          one steady eager StreamReceiver(batch=1).push, and solo_total_ms = S times that: one session object per
                       session, the only way to serve independent sessions without the pool; round_over_solo = (b) / (S * (d)).
The two ratios are reported, not gated.  Timing: torch.cuda events around each call (they bracket the host work too) after
--warmup rounds in the steady state; --repeats rounds are timed, (c) and (d) as many calls.  Every timed call decodes a real next
chunk of a session that keeps running (the packets of one chunk are re-numbered on the host for each).  Seeded synthetic weights
and signals: only the times mean anything.

With --decoder stateful every row also carries "stateful": the same rounds on StreamReceiverPool(decoder="stateful") (DESIGN.md
section 23), measured in the same run right after the window-mode pool's, and window_round_over_stateful_round.

  python tools/stream_pool_bench.py [--repeats 10] [--warmup 3] [--sessions 1,6,64,256] [--decoder window|stateful]
"""
import argparse
import json
import statistics
import struct
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K = 8, 512
CHUNK_MS = 16 / 75 * 1000.0
ROUND = 16                                                            # ticks per chunk: one per token-time


def renumber(pkt, seq):
    """The same packet under another sequence number (the header's uint32 at offset 3)."""
    return pkt[:3] + struct.pack("<I", seq) + pkt[7:]


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def pool_rounds(net, chunk, codes, S, warmup, repeats, **kw):
    """-> (per-round sums, the times of the ticks that served a session) of `repeats` steady rounds."""
    pool = net.stream_receiver_pool(K, BOOKS, slots=S, **kw)
    sids = [pool.open() for _ in range(S)]

    def tick(t):
        pushes = {}
        for i in range(t % ROUND, S, ROUND):
            base = pool.tokens(sids[i]) // 2
            pushes[sids[i]] = ([renumber(p, base + j) for j, p in enumerate(chunk[i])], codes[i])
        return pushes

    t = 0
    for _ in range((2 + warmup) * ROUND):                             # two rounds reach the steady state (16, 32 tokens), then warm-up
        pool.step(tick(t))
        t += 1
    torch.cuda.synchronize()
    assert all(pool.tokens(s) == 16 * (2 + warmup) for s in sids)
    rounds, served = [], []
    for _ in range(repeats):
        total = 0.0
        for _ in range(ROUND):
            pushes = tick(t)                                          # choosing and re-numbering the packets is the caller's work
            ms = event_ms(lambda: pool.step(pushes))
            total += ms
            if pushes:
                served.append(ms)
            t += 1
        rounds.append(total)
    for s in sids:
        pool.close(s)
    return rounds, served


def lockstep_steps(net, chunk, codes, B, warmup, repeats):
    """`repeats` steady eager pushes of a StreamReceiver(batch=B) on the first B sessions' chunks."""
    rx = net.stream_receiver(K, BOOKS, batch=B)
    c = {"n": 0}

    def push():
        n = c["n"]
        c["n"] += 1
        return rx.push([[renumber(p, 8 * n + j) for j, p in enumerate(item)] for item in chunk[:B]], codes[:B])
    for _ in range(2 + warmup):
        push()
    torch.cuda.synchronize()
    return [event_ms(push) for _ in range(repeats)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sessions", default="1,6,64,256")
    ap.add_argument("--decoder", choices=("window", "stateful"), default="window",
                    help="stateful: also measure StreamReceiverPool(decoder='stateful') in the same run")
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from multimodal_vqvae_compression_audio_tactile_amd import bitstream, build_proposed, synth
    if not torch.cuda.is_available():
        raise SystemExit("stream_pool_bench: needs an MI355X (a time measured anywhere else says nothing)")
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    sizes = [int(s) for s in args.sessions.split(",")]
    out = {"books": BOOKS, "K": K, "packet_tok": 2, "chunk_tok": 16, "ticks_per_round": ROUND, "chunk_ms": CHUNK_MS,
           "repeats": args.repeats, "warmup": args.warmup, "rows": []}
    with torch.no_grad():
        S_max = max(sizes)
        a, t = synth.audio_segments(S_max, seed=11).to(dev), synth.tactile_segments(S_max, seed=11).to(dev)
        _, pk, aud = net.compress_packets(a, t)
        codes = torch.from_numpy(np.stack([bitstream.unpack_indices(p)[0] for p in aud]))[..., 16:32].contiguous()
        chunk = [item[8:16] for item in pk]                           # the packets of tokens 16..31
        solo = spread(lockstep_steps(net, chunk, codes, 1, args.warmup, args.repeats))
        for S in sizes:
            rounds, served = pool_rounds(net, chunk, codes, S, args.warmup, args.repeats)
            lock = spread(lockstep_steps(net, chunk, codes, S, args.warmup, args.repeats))
            row = {"S": S, "sessions_per_tick": S / ROUND, "tick_ms": spread(served), "round_ms": spread(rounds),
                   "lockstep_ms": lock, "solo_ms": solo, "solo_total_ms": S * solo["median"]}
            row["round_over_lockstep"] = row["round_ms"]["median"] / lock["median"]
            row["round_over_solo"] = row["round_ms"]["median"] / row["solo_total_ms"]
            row["real_time_factor"] = row["round_ms"]["median"] / CHUNK_MS
            if args.decoder == "stateful":
                r2, s2 = pool_rounds(net, chunk, codes, S, args.warmup, args.repeats, decoder="stateful")
                row["stateful"] = {"tick_ms": spread(s2), "round_ms": spread(r2)}
                row["window_round_over_stateful_round"] = row["round_ms"]["median"] / row["stateful"]["round_ms"]["median"]
            out["rows"].append(row)
    print(json.dumps(out))
    slow = [r["S"] for r in out["rows"] if r["round_ms"]["median"] >= CHUNK_MS]
    if slow:
        raise SystemExit(f"the pool does not keep up with real time at S = {slow}: 16 ticks take longer than the {CHUNK_MS:.1f} ms they decode")


if __name__ == "__main__":
    main()
