#!/usr/bin/env python3
"""The receiver's audio output on the MI355X: one JSON line with, per batch size B (one-second segments,
T_lat = 75, 8 tactile books x K = 512, 32 audio stages x K = 1024, packets of 2 tokens; every other audio packet of chunk 1 and one
packet of every other chunk lost; fade = AudioFade(1, 4); the audio decoder carries seeded weights):
    fade_ms                       ops.audio_fade_ alone: the steady piece [B, 1, 5120] with its state, and the whole item [B, 1, 23992];
    decompress_av_ms              decompress_packets_av with audio_out False / True;
    recv_step_ms / _graph_ms      the StreamReceiver(audio=(1024, 32)) steady step (a 16-token push onto a full history), eager and
                                  graph=True, decoder "window" / "stateful", audio_out False / True;
    pool_round_ms                 16 ticks of a StreamReceiverPoolAV in which every one of S sessions (--sessions) pushes a chunk,
                                  audio_out False / True (one event pair around the 16 ticks);
each --a-runs times, audio_out False and True alternating.  The audio_out=False rows -- decompress_packets_av and the steady steps,
no audio_out argument anywhere -- are ALSO measured in fresh child processes, --a-runs of this tree and, with --a-root, as many of
a built checkout of the parent commit, alternating the two trees: the spread of the parent's runs is the margin within which this
tree did or did not move.  Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events
bracket host work too.

  python tools/audio_out_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--sessions 1,6,64,256] [--a-root PATH] [--a-runs 3]
"""
import argparse
import json
import statistics
import struct
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K, PTOK, AUDIO = 8, 512, 2, (1024, 32)
DECODERS = ("window", "stateful")
TICKS = 16


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


def _net(dev, audio_decoder=False):
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    if audio_decoder:
        from multimodal_vqvae_compression_audio_tactile_amd import DAC
        dec = DAC().decoder
        dec.load_state_dict(synth.decoder_state(234), strict=True)
        net.set_audio_decoder(dec)
    return net


def inputs(B, dev):
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    return synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)


def timing_loss(apk):
    """The audio packets that arrive in the timed runs: per item every other packet of chunk 1 and packet 8c + 3 of every other
    chunk are lost."""
    drop = lambda s: (8 <= s < 16 and s % 2 == 1) or (not 8 <= s < 16 and s % 8 == 3)
    return [[p for s, p in enumerate(lst) if not drop(s)] for lst in apk]


def _chunks(lists, B, n):
    """Per item the packets of chunk 1 that arrive, re-stamped as chunk c for c < n."""
    per = 16 // PTOK
    seq = lambda p: int.from_bytes(bytes(p)[3:7], "little")
    stamp = lambda p, c: bytes(p[:3]) + struct.pack("<I", per * c + seq(p) - per) + bytes(p[7:])
    return [[[stamp(p, c) for p in lists[b] if per <= seq(p) < 2 * per] for b in range(B)] for c in range(n)]


def steady_recv(net, B, pk, apk, n_push, graph, **kw):
    """A receiver session with a full history -> the function that pushes its next chunk."""
    rx = net.stream_receiver(K, BOOKS, batch=B, graph=graph, audio=AUDIO, **kw)
    tp, ap = _chunks(pk, B, n_push), _chunks(apk, B, n_push)
    state = {"c": 0}

    def push():
        c = state["c"]
        state["c"] += 1
        return rx.push(tp[c], ap[c])
    push(), push(), push()                                               # the two shorter windows, then the steady shape (the capture)
    return push


def pool_round(net, S, pk, apk, **kw):
    """-> the function that opens S sessions on a fresh StreamReceiverPoolAV and runs TICKS ticks in which each pushes a chunk."""
    from multimodal_vqvae_compression_audio_tactile_amd.stream import StreamReceiverPoolAV
    tp, ap = _chunks(pk, S, TICKS), _chunks(apk, S, TICKS)
    pool = StreamReceiverPoolAV(net, K, BOOKS, slots=S, audio=AUDIO, **kw)

    def run():
        sids = [pool.open() for _ in range(S)]
        for c in range(TICKS):
            pool.step({sid: (tp[c][b], ap[c][b]) for b, sid in enumerate(sids)})
        for sid in sids:
            pool.close(sid)
    return run


def old_rows(args):
    """The audio_out=False paths on whatever package sys.path resolves to (no audio_out argument anywhere)."""
    dev = torch.device("cuda:0")
    net = _net(dev)
    rows, n_push = {}, 3 + args.warmup + args.repeats
    w, r = args.warmup, args.repeats
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev)
            infos, pk, ainfos, apk = net.compress_packets_av(a, t)
            arx = timing_loss(apk)
            row = {"decompress_av_ms": timed(lambda: net.decompress_packets_av(infos, pk, ainfos, arx), w, r)}
            for dec in DECODERS:
                row[f"recv_step_{dec}_ms"] = timed(steady_recv(net, B, pk, arx, n_push, False, decoder=dec), w, r)
                row[f"recv_step_{dec}_graph_ms"] = timed(steady_recv(net, B, pk, arx, n_push, True, decoder=dec), w, r)
            rows[B] = row
    return rows


def child(args, root):
    """One fresh child process measuring the audio_out=False paths of the package under ``root``."""
    c = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--old-only", "--root", str(root), "--repeats",
                        str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                       capture_output=True, text=True, timeout=900)
    if c.returncode != 0:
        raise SystemExit(f"measuring {root} failed:\n" + c.stdout[-2000:] + c.stderr[-2000:])
    return {int(k): v for k, v in json.loads(c.stdout.strip().splitlines()[-1])["old"].items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--sessions", default="1,6,64,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: the audio_out=False paths are also measured on it, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--old-only", action="store_true", help="internal: print the audio_out=False rows for the package under --root and exit")
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
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    from multimodal_vqvae_compression_audio_tactile_amd.packets import AudioFade
    dev = torch.device("cuda:0")
    net = _net(dev, audio_decoder=True)
    fade = AudioFade(1, 4)
    out = {"books": BOOKS, "K": K, "T_lat": 75, "packet_tok": PTOK, "fade": [1, 4], "repeats": args.repeats, "warmup": args.warmup,
           "rows": [], "pool": []}
    w, r = args.warmup, args.repeats
    n_push = 3 + w + r
    med = lambda res: {k: {"runs": v, "median": statistics.median(v)} for k, v in res.items()}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev)
            row = {"B": B, "existing": {}}
            for key in (here[0][B] if here else {}):
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
            # the kernel alone: a steady piece (tokens 22..38 of a session at 32 tokens) and the whole item
            nav = torch.full((B, 75), 32, dtype=torch.uint8, device=dev)
            nav[:, 17:32:4] = 0
            nav[:, 18:32:4] = 0
            piece, whole = torch.randn(B, 1, 5120, device=dev), torch.randn(B, 1, 320 * 75 - 8, device=dev)
            st, v16 = ops.audio_fade_state(B, dev), nav[:, 16:32].contiguous()
            row["fade_ms"] = {"piece_5120": timed(lambda: ops.audio_fade_(piece, v16, st, fade, 22), w, r),
                              "whole_23992": timed(lambda: ops.audio_fade_(whole, nav, st, fade, 0), w, r)}
            res = {False: {}, True: {}}
            for _ in range(args.a_runs):                                     # off and on alternate: a drift of the box hits both
                for on in (False, True):
                    kw = dict(audio_out=True, audio_fade=fade) if on else {}
                    m = {"decompress_av_ms": timed(lambda: net.decompress_packets_av(infos, pk, ainfos, arx, **kw), w, r)}
                    for dec in DECODERS:
                        m[f"recv_step_{dec}_ms"] = timed(steady_recv(net, B, pk, arx, n_push, False, decoder=dec, **kw), w, r)
                        m[f"recv_step_{dec}_graph_ms"] = timed(steady_recv(net, B, pk, arx, n_push, True, decoder=dec, **kw), w, r)
                    for k, v in m.items():
                        res[on].setdefault(k, []).append(v)
            row["audio_out_off"], row["audio_out_on"] = med(res[False]), med(res[True])
            out["rows"].append(row)
        for S in (int(s) for s in args.sessions.split(",") if s):
            a, t = inputs(S, dev)
            infos, pk, ainfos, apk = net.compress_packets_av(a, t)
            arx = timing_loss(apk)
            res = {False: {}, True: {}}
            for _ in range(args.a_runs):
                for on in (False, True):
                    kw = dict(audio_out=True, audio_fade=fade) if on else {}
                    for dec in DECODERS:
                        res[on].setdefault(f"pool_round_{dec}_ms", []).append(timed(pool_round(net, S, pk, arx, decoder=dec, **kw), 1, max(1, r // 3)))
            out["pool"].append({"sessions": S, "ticks": TICKS, "audio_out_off": med(res[False]), "audio_out_on": med(res[True])})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
