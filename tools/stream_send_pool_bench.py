#!/usr/bin/env python3
"""The sender pool on the MI355X: one JSON line with, per number of sessions S (1 / 6 / 64 / 256; 8 books
x K = 512, packets of 2 tokens), all in this one process,
  (a) tick_emit_ms     one StreamSenderPool.step, host work included, of a tick in which sessions emit.  Session i starts
                       (i mod 16) token-times late, there is one tick per token-time (13.3 ms of signal) and EVERY session pushes
                       one token (320 samples of each modality) in every tick: a tick appends for all S sessions and encodes a
                       chunk for the sessions whose 24th, 40th, 56th ... token it brought -- those with i mod 16 == (tick - 23)
                       mod 16, about S/16 of them, all in the steady group (32-token window) once each has two chunks behind it.
                       Median, minimum and maximum over the timed ticks that emitted;
  (b) tick_append_ms   the tick that only appends (one sample-state launch for all S sessions, no read-back).  With S >= 16 the
                       staggered workload has none, so it is timed on a second pool whose S sessions started together: 15 of its
                       16 ticks append only;
  (c) round_ms         the sum of 16 consecutive ticks of (a)'s workload: every one of the S sessions pushed 16 tokens and emitted
                       one chunk, 213.3 ms of signal.  Median, minimum and maximum over the timed rounds.  THE THRESHOLD: the
                       median must stay under 213.3 ms;
  (d) lockstep_ms      one steady eager StreamSender(batch=S).push of 16 tokens -- the same S chunks as ONE batch, which needs the
                       S sessions in lockstep; and round_over_lockstep = (c) / (d), what serving them out of step costs;
  (e) solo_ms          one steady eager StreamSender(batch=1).push of 16 tokens, and solo_total_ms = S times that: one session
                       object per session, the only way to serve independent sessions without the pool (it leaves out the 15
                       append launches per chunk that a solo session fed token by token also pays); round_over_solo = (c) / (S * (e)).
  (f) --encoder stateful   the pool (and (d), (e)) with encoder="stateful" (DESIGN.md section 24); "both": the rows of both modes
                       in this one process, each row tagged "encoder".
  (g) --link av        the same rows on StreamSenderPoolAV: both streams rate-controlled, the audio codes in
                       layered packets, with --fec also Fec(4, 3) on the tactile and Fec(8, 4, 2) on the audio stream; (d) and (e)
                       are StreamSender with the same options.  Each row also carries "plain_round_ms", the plain pool's round in
                       the same run, and "host_ms" / "frame_ms": the host time of a round's 16 step calls (time.perf_counter; it
                       includes the wait for the tick's one read-back) and the part of it spent framing packets.
The two ratios are reported, not gated.  The samples of every call are HOST tensors, as they arrive, in all three.  Timing:
torch.cuda events around each call (they bracket the host work too) after --warmup rounds in the steady state; --repeats rounds
are timed, (d) and (e) as many calls.  Every timed call encodes real next samples of sessions that keep running (a 1-s signal per
session, repeated).  Seeded synthetic weights and signals: only the times mean anything.

  python tools/stream_send_pool_bench.py [--repeats 10] [--warmup 3] [--sessions 1,6,64,256] [--encoder window|stateful|both]
                                         [--link plain|av [--fec]]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K = 8, 512
CHUNK_MS = 16 / 75 * 1000.0
ROUND = 16                                                            # ticks per chunk: one per token-time
HOP = 320
SIGNAL_TOK = 75                                                       # the 1-s signal of a session repeats


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)} if ms else None


def enc_kw(encoder):
    return {} if encoder == "window" else {"encoder": encoder}


def av_kw(fec):
    """The options of --link av, for the pool and the lockstep sender alike."""
    from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, Rate
    kw = dict(rate=Rate(min_books=2, tol2=0.84), audio="packets", audio_rate=Rate(min_books=2, tol2=0.5))
    return dict(kw, fec=Fec(4, 3), audio_fec=Fec(8, 4, 2)) if fec else kw


def pool_ticks(net, a, t, S, stagger, warmup, repeats, encoder="window", av=None, host=None):
    """A pool of S sessions, session i starting (i mod 16 if ``stagger`` else 0) ticks late, every open session pushing one token
    per tick.  -> (per-round sums, the times of the ticks that emitted, the times of the ticks that only appended) of
    ``repeats`` steady rounds.  ``av``: the options of a StreamSenderPoolAV; ``host``: a dict that receives the host times per round."""
    import time
    pool = net.stream_sender_pool(slots=S, **enc_kw(encoder)) if av is None else net.stream_sender_pool_av(slots=S, **av, **enc_kw(encoder))
    spent = {"frame": 0.0, "step": 0.0}
    if host is not None:
        frame = pool._frame

        def timed_frame(*args):
            t0 = time.perf_counter()
            try:
                return frame(*args)
            finally:
                spent["frame"] += time.perf_counter() - t0
        pool._frame = timed_frame
    late = [i % ROUND if stagger else 0 for i in range(S)]
    sids, fed = {}, [0] * S

    def tick(now):
        pushes = {}
        for i in range(S):
            if late[i] == now:
                sids[i] = pool.open()
            if late[i] <= now:
                at = HOP * (fed[i] % SIGNAL_TOK)
                pushes[sids[i]] = (a[i:i + 1, :, at:at + HOP], t[i:i + 1, :, at:at + HOP])
                fed[i] += 1
        return pushes

    now = 0
    for _ in range((4 + warmup) * ROUND):                             # four rounds: every session is past its second chunk
        pool.step(tick(now))
        now += 1
    torch.cuda.synchronize()
    assert all(pool._sess[s][3] >= 2 for s in sids.values())
    rounds, emit, append = [], [], []
    for _ in range(repeats):
        total = 0.0
        for _ in range(ROUND):
            pushes = tick(now)                                        # slicing the signals is the caller's work
            got = {}
            t0 = time.perf_counter()
            ms = event_ms(lambda: got.update(pool.step(pushes)))
            spent["step"] += time.perf_counter() - t0
            total += ms
            (emit if any(v[0] for v in got.values()) else append).append(ms)
            now += 1
        rounds.append(total)
    if host is not None:
        host.update(host_ms=1e3 * spent["step"] / repeats, frame_ms=1e3 * spent["frame"] / repeats)
    for s in sids.values():
        pool.close(s)
    return rounds, emit, append


def lockstep_steps(net, a, t, B, warmup, repeats, encoder="window", av=None):
    """``repeats`` steady eager 16-token pushes of a StreamSender(batch=B) on the first B sessions' signals."""
    tx = net.stream_sender(batch=B, **(av or {}), **enc_kw(encoder))
    c = {"n": 0}
    n_steps = a.shape[-1] // (ROUND * HOP)

    def push():
        at = ROUND * HOP * (c["n"] % n_steps)
        c["n"] += 1
        return tx.push(a[:B, :, at:at + ROUND * HOP], t[:B, :, at:at + ROUND * HOP])
    for _ in range(3 + warmup):                                       # nothing, chunk 0 (24-token window), the first steady step
        push()
    torch.cuda.synchronize()
    return [event_ms(push) for _ in range(repeats)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sessions", default="1,6,64,256")
    ap.add_argument("--encoder", default="window", choices=("window", "stateful", "both"))
    ap.add_argument("--link", choices=("plain", "av"), default="plain", help="av: StreamSenderPoolAV on both streams (section 25)")
    ap.add_argument("--fec", action="store_true", help="--link av: Fec(4, 3) on the tactile and Fec(8, 4, 2) on the audio stream")
    args = ap.parse_args()
    if args.fec and args.link != "av":
        raise SystemExit("stream_send_pool_bench: --fec goes with --link av")
    sys.path.insert(0, str(ROOT))
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    if not torch.cuda.is_available():
        raise SystemExit("stream_send_pool_bench: needs an MI355X (a time measured anywhere else says nothing)")
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    sizes = [int(s) for s in args.sessions.split(",")]
    out = {"books": BOOKS, "K": K, "packet_tok": 2, "chunk_tok": 16, "ticks_per_round": ROUND, "chunk_ms": CHUNK_MS,
           "repeats": args.repeats, "warmup": args.warmup, "rows": []}
    with torch.no_grad():
        S_max = max(sizes)
        a, t = synth.audio_segments(S_max, seed=11), synth.tactile_segments(S_max, seed=11)        # on the host, [S, 1, 24000]
        assert a.shape[-1] == SIGNAL_TOK * HOP and not a.is_cuda
        modes = ("window", "stateful") if args.encoder == "both" else (args.encoder,)
        av = av_kw(args.fec) if args.link == "av" else None
        if av is not None:
            out.update(link="av", fec=args.fec)
        solos = {m: spread(lockstep_steps(net, a, t, 1, args.warmup, args.repeats, m, av)) for m in modes}
        for S, mode in ((S, m) for S in sizes for m in modes):
            solo = solos[mode]
            host = {} if av is not None else None
            rounds, emit, append = pool_ticks(net, a, t, S, True, args.warmup, args.repeats, mode, av, host)
            if S >= ROUND:                                            # every tick of the staggered workload emits
                append = pool_ticks(net, a, t, S, False, 0, max(1, args.repeats // 5), mode, av)[2]
            lock = spread(lockstep_steps(net, a, t, S, args.warmup, args.repeats, mode, av))
            row = {"S": S, "encoder": mode, "emitting_per_tick": S / ROUND, "tick_emit_ms": spread(emit), "tick_append_ms": spread(append),
                   "round_ms": spread(rounds), "lockstep_ms": lock, "solo_ms": solo, "solo_total_ms": S * solo["median"]}
            if av is not None:
                plain = spread(pool_ticks(net, a, t, S, True, args.warmup, args.repeats, mode)[0])
                row.update(plain_round_ms=plain, round_over_plain=row["round_ms"]["median"] / plain["median"], **host)
            row["round_over_lockstep"] = row["round_ms"]["median"] / lock["median"]
            row["round_over_solo"] = row["round_ms"]["median"] / row["solo_total_ms"]
            row["real_time_factor"] = row["round_ms"]["median"] / CHUNK_MS
            out["rows"].append(row)
    print(json.dumps(out))
    slow = [r["S"] for r in out["rows"] if r["round_ms"]["median"] >= CHUNK_MS]
    if slow:
        raise SystemExit(f"the pool does not keep up with real time at S = {slow}: 16 ticks take longer than the {CHUNK_MS:.1f} ms they encode")


if __name__ == "__main__":
    main()
