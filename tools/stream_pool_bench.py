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

With --link av the rows are those of StreamReceiverPoolAV on the whole link -- the audio codes arrive as
layered packets (32 stages, both streams rate-controlled at the sender), with --fec also Fec(4, 3) on the tactile and Fec(8, 4, 2)
on the audio stream (every parity packet arrives, nothing is lost: the recovery launches run and repair nothing), with
--audio-conceal the mode -- against StreamReceiver(batch=S / 1) with the same options; each row also carries "plain_round_ms", the
plain pool's round in the same run, and "host_ms" / "gather_ms": the host time of a round's 16 step calls (time.perf_counter; the
receiver reads nothing back, so it is the host's share) and the part of it spent gathering packets.

  python tools/stream_pool_bench.py [--repeats 10] [--warmup 3] [--sessions 1,6,64,256] [--decoder window|stateful]
                                    [--link plain|av [--fec] [--audio-conceal zero|mask|hold]]
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


def av_chunk(av, i, base):
    """Session i's chunk of the whole link under the sequence numbers from ``base`` on: (packets, audio packets, parity, audio
    parity); a parity packet carries its group's number (groups of 4 and of 8 packets; two parity packets per audio group)."""
    pk, apk, par, apar = av
    return ([renumber(p, base + j) for j, p in enumerate(pk[i])], [renumber(p, base + j) for j, p in enumerate(apk[i])],
            None if par is None else [renumber(p, base // 4 + j) for j, p in enumerate(par[i])],
            None if apar is None else [renumber(p, base // 8 + j // 2) for j, p in enumerate(apar[i])])


def pool_rounds(net, chunk, codes, S, warmup, repeats, av=None, host=None, **kw):
    """-> (per-round sums, the times of the ticks that served a session) of `repeats` steady rounds.  ``av``: the chunk of the
    whole link (StreamReceiverPoolAV with the options ``kw``); ``host``: a dict that receives the host times per round."""
    import time
    pool = net.stream_receiver_pool(K, BOOKS, slots=S, **kw) if av is None else net.stream_receiver_pool_av(K, BOOKS, slots=S, **kw)
    sids = [pool.open() for _ in range(S)]
    spent = {"gather": 0.0, "step": 0.0}
    if host is not None:
        inputs = pool._inputs

        def timed_inputs(*a):
            t0 = time.perf_counter()
            try:
                return inputs(*a)
            finally:
                spent["gather"] += time.perf_counter() - t0
        pool._inputs = timed_inputs

    def tick(t):
        pushes = {}
        for i in range(t % ROUND, S, ROUND):
            base = pool.tokens(sids[i]) // 2
            if av is not None:
                pushes[sids[i]] = av_chunk(av, i, base)
            else:
                pushes[sids[i]] = ([renumber(p, base + j) for j, p in enumerate(chunk[i])], codes[i])
        return pushes

    def step(pushes):
        t0 = time.perf_counter()
        pool.step(pushes)
        spent["step"] += time.perf_counter() - t0

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
            ms = event_ms(lambda: step(pushes))
            total += ms
            if pushes:
                served.append(ms)
            t += 1
        rounds.append(total)
    if host is not None:
        host.update(host_ms=1e3 * spent["step"] / repeats, gather_ms=1e3 * spent["gather"] / repeats)
    for s in sids:
        pool.close(s)
    return rounds, served


def lockstep_steps(net, chunk, codes, B, warmup, repeats, av=None, **kw):
    """`repeats` steady eager pushes of a StreamReceiver(batch=B) on the first B sessions' chunks (``av``: of the whole link)."""
    rx = net.stream_receiver(K, BOOKS, batch=B, **kw)
    c = {"n": 0}

    def push():
        n = c["n"]
        c["n"] += 1
        if av is not None:
            tp, ap, fp, afp = zip(*(av_chunk(av, i, 8 * n) for i in range(B)))
            return rx.push(list(tp), audio_packets=list(ap), fec_packets=None if fp[0] is None else list(fp),
                           audio_fec_packets=None if afp[0] is None else list(afp))
        return rx.push([[renumber(p, 8 * n + j) for j, p in enumerate(item)] for item in chunk[:B]], codes[:B])
    for _ in range(2 + warmup):
        push()
    torch.cuda.synchronize()
    return [event_ms(push) for _ in range(repeats)]


def av_rows(net, a, t, chunk, codes, sizes, args, out):
    """The rows of --link av: the staggered round on StreamReceiverPoolAV against the plain pool's round, the lockstep AV step and
    S solo AV sessions."""
    from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, Rate
    fec, afec = (Fec(4, 3), Fec(8, 4, 2)) if args.fec else (None, None)
    sent = net.compress_packets_av(a, t, rate=Rate(min_books=2, tol2=0.84), audio_rate=Rate(min_books=2, tol2=0.5), fec=fec, audio_fec=afec)
    pk, apk = sent[1], sent[3]
    av = ([item[8:16] for item in pk], [item[8:16] for item in apk],                      # the packets of tokens 16..31, their groups
          [item[2:4] for item in sent[4]] if args.fec else None, [item[2:4] for item in sent[5]] if args.fec else None)
    kw = dict(audio=(1024, 32), fec=fec, audio_fec=afec, audio_conceal=args.audio_conceal)
    out.update(link="av", fec=args.fec, audio_conceal=args.audio_conceal)
    solo = spread(lockstep_steps(net, None, None, 1, args.warmup, args.repeats, av=av, **kw))
    for S in sizes:
        host = {}
        rounds, served = pool_rounds(net, None, None, S, args.warmup, args.repeats, av=av, host=host, **kw)
        plain, _ = pool_rounds(net, chunk, codes, S, args.warmup, args.repeats)
        lock = spread(lockstep_steps(net, None, None, S, args.warmup, args.repeats, av=av, **kw))
        row = {"S": S, "sessions_per_tick": S / ROUND, "tick_ms": spread(served), "round_ms": spread(rounds), "plain_round_ms": spread(plain),
               "lockstep_ms": lock, "solo_ms": solo, "solo_total_ms": S * solo["median"], **host}
        row["round_over_plain"] = row["round_ms"]["median"] / row["plain_round_ms"]["median"]
        row["round_over_lockstep"] = row["round_ms"]["median"] / lock["median"]
        row["round_over_solo"] = row["round_ms"]["median"] / row["solo_total_ms"]
        row["real_time_factor"] = row["round_ms"]["median"] / CHUNK_MS
        out["rows"].append(row)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sessions", default="1,6,64,256")
    ap.add_argument("--decoder", choices=("window", "stateful"), default="window",
                    help="stateful: also measure StreamReceiverPool(decoder='stateful') in the same run")
    ap.add_argument("--link", choices=("plain", "av"), default="plain", help="av: StreamReceiverPoolAV on audio packets (section 25)")
    ap.add_argument("--fec", action="store_true", help="--link av: Fec(4, 3) on the tactile and Fec(8, 4, 2) on the audio stream")
    ap.add_argument("--audio-conceal", choices=("zero", "mask", "hold"), default="zero", help="--link av: the receiver's mode")
    args = ap.parse_args()
    if args.link != "av" and (args.fec or args.audio_conceal != "zero"):
        raise SystemExit("stream_pool_bench: --fec / --audio-conceal go with --link av")
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
        if args.link == "av":
            av_rows(net, a, t, chunk, codes, sizes, args, out)
            sizes = []
        solo = spread(lockstep_steps(net, chunk, codes, 1, args.warmup, args.repeats)) if sizes else None
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
