#!/usr/bin/env python3
"""Forward error correction on the MI355X: one JSON line with, per batch size B (1 / 6 / 256 one-second segments, T_lat = 75, 8 tactile
books x K = 512, 32 audio stages x K = 1024, packets of 2 tokens, Fec(4, 3) on the tactile and Fec(4, 4) on the audio stream),
  (a) existing                 compress_packets / decompress_packets, compress_packets_av / decompress_packets_av and the sender and
                               receiver steady steps (eager and graph=True, both streams as packets) with the new arguments at None,
                               measured in fresh child processes: --a-runs of this tree and, with --a-root, as many of a built
                               checkout of the parent commit -- the spread of each side's runs is the margin within which the other
                               side did or did not move;
  (b) fec                      the same calls with the two Fec on;
  (c) kernel_us                the two kernels' own times, from the library's profile events (fec_parity_kernel, fec_recover_kernel);
  (d) overhead_kbps            what the parity packets add, bodies / with headers (packets.fec_kbps), next to the data streams';
  (e) loss                     over a seeded channel at 5 / 10 / 20 % independent packet loss (data and parity alike), per stream the
                               share of lost packets recovered, and per chunk index the max |z_run(sender) - z_run(receiver)| over the
                               batch with and without FEC.
  --parity G:R[,G:R...]        extra codes Fec(G, 3, R) + Fec(G, 4, R) (Reed-Solomon for R > 1): out["parity"] gets, per code, (b) to
                               (e) again -- the kernel times then name fec_rs_parity_kernel / fec_rs_recover_kernel.  Without the
                               option the output is what it was.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  Seeded
synthetic weights and signals: the times mean something, the recovered shares follow from the loss model alone, and the drift
exercises plumbing only.

  python tools/fec_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH] [--a-runs 3] [--parity 8:2,4:2]
"""
import argparse
import json
import statistics
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K, PTOK, KA, STAGES = 8, 512, 2, 1024, 32
STEP = 5120
KEYS = ("compress_ms", "decompress_ms", "compress_av_ms", "decompress_av_ms", "step_ms", "step_graph_ms", "recv_step_ms", "recv_step_graph_ms")


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


def steady_push(net, a, t, B, graph, **kw):
    """A sender session in its steady state -> the function that pushes its next 16 tokens (the 1-s signal repeats)."""
    tx = net.stream_sender(batch=B, graph=graph, audio="packets", **kw)
    n_steps, state = a.shape[-1] // STEP, {"c": 0}

    def push():
        c = state["c"] % n_steps
        state["c"] += 1
        return tx.push(a[..., STEP * c:STEP * (c + 1)], t[..., STEP * c:STEP * (c + 1)])
    push(), push(), push()
    return push


def steady_recv(net, B, sent, n_push, graph, fecs=None):
    """A receiver session with a full history -> the function that pushes its next chunk.  ``sent``: compress_packets_av's return
    value; chunk 1's packets (and parity groups) serve every push, re-stamped with the push's sequence numbers beforehand."""
    rx = net.stream_receiver(K, BOOKS, batch=B, graph=graph, audio=(KA, STAGES), **({} if fecs is None else {"fec": fecs[0], "audio_fec": fecs[1]}))
    stamp = lambda p, seq: bytes(p[:3]) + struct.pack("<I", seq) + bytes(p[7:])

    def chunk(lists, c, per, r=1):                                      # ``per`` numbers per chunk, r packets under each (parity)
        return [[stamp(p, per * c + i // r) for i, p in enumerate(lists[b][per * r:2 * per * r])] for b in range(B)]
    per = 16 // PTOK
    pushes = []
    for c in range(n_push):
        kw = {"audio_packets": chunk(sent[3], c, per)}
        if fecs is not None:
            kw.update(fec_packets=chunk(sent[4], c, per // fecs[0].group, fecs[0].parity),
                      audio_fec_packets=chunk(sent[5], c, per // fecs[1].group, fecs[1].parity))
        pushes.append((chunk(sent[1], c, per), kw))
    state = {"c": 0}

    def push():
        tp, kw = pushes[state["c"]]
        state["c"] += 1
        return rx.push(tp, **kw)
    push(), push(), push()                                               # the two shorter windows, then the steady shape (the capture)
    return push


def _net(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    return build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)


def rows_of(net, args, synth, fecs=None):
    """Every timed call, with the two Fec (``fecs``) or with the new arguments left out (which is what a parent tree accepts)."""
    dev = torch.device("cuda:0")
    rows, n_push = {}, 3 + args.warmup + args.repeats
    kw1 = {} if fecs is None else {"fec": fecs[0]}
    kw2 = {} if fecs is None else {"fec": fecs[0], "audio_fec": fecs[1]}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)
            s1, s2 = net.compress_packets(a, t, **kw1), net.compress_packets_av(a, t, **kw2)
            d1 = (lambda: net.decompress_packets(*s1)) if fecs is None else (lambda: net.decompress_packets(*s1[:3], fec=fecs[0], fec_packets=s1[3]))
            d2 = (lambda: net.decompress_packets_av(*s2)) if fecs is None else \
                (lambda: net.decompress_packets_av(*s2[:4], fec=fecs[0], fec_packets=s2[4], audio_fec=fecs[1], audio_fec_packets=s2[5]))
            rows[B] = {"compress_ms": timed(lambda: net.compress_packets(a, t, **kw1), args.warmup, args.repeats),
                       "decompress_ms": timed(d1, args.warmup, args.repeats),
                       "compress_av_ms": timed(lambda: net.compress_packets_av(a, t, **kw2), args.warmup, args.repeats),
                       "decompress_av_ms": timed(d2, args.warmup, args.repeats),
                       "step_ms": timed(steady_push(net, a, t, B, False, **kw2), args.warmup, args.repeats),
                       "step_graph_ms": timed(steady_push(net, a, t, B, True, **kw2), args.warmup, args.repeats),
                       "recv_step_ms": timed(steady_recv(net, B, s2, n_push, False, fecs), args.warmup, args.repeats),
                       "recv_step_graph_ms": timed(steady_recv(net, B, s2, n_push, True, fecs), args.warmup, args.repeats)}
    return rows


def children(args, roots):
    """``--a-runs`` fresh child processes per tree measuring the existing paths of the package under each of ``roots``, the trees
    alternating (so a drift of the machine over the call lands on both) -> one list of runs per tree."""
    return [list(runs) for runs in zip(*([child_run(args, root) for root in roots] for _ in range(args.a_runs)))] or [[] for _ in roots]


def child_run(args, root):
    child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--old-only", "--root", str(root), "--repeats",
                            str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                           capture_output=True, text=True, timeout=900)
    if child.returncode != 0:
        raise SystemExit(f"measuring {root} failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
    return {int(k): v for k, v in json.loads(child.stdout.strip().splitlines()[-1])["old"].items()}


def loss_rows(net, a, t, fecs, rates, seed, packets):
    """(e): the closed-loop sender's z_run against the receiver's over a seeded channel, with and without recovery."""
    dev = a.device
    B = a.shape[0]
    z_run, codes, idx, nb_sent, na_sent = net.encode_latents_with_indices(a, t, rate=packets.Rate(), audio_rate=packets.Rate())
    sent = net.compress_packets_av(a, t, fec=fecs[0], audio_fec=fecs[1])
    info, ainfo = sent[0][0], sent[2][0]
    out = {}
    for rate in rates:
        r = np.random.default_rng(seed + int(1000 * rate))
        keep = lambda lists: [[p for p in lists[b] if r.uniform() >= rate] for b in range(B)]
        rx, arx, rxp, arxp = keep(sent[1]), keep(sent[3]), keep(sent[4]), keep(sent[5])
        arrays, share = {}, {}
        for name, inf, f, data, par in (("tactile", info, fecs[0], rx, rxp), ("audio", ainfo, fecs[1], arx, arxp)):
            plain, fixed, lost, rec = [], [], 0, 0
            for b in range(B):
                bodies, counts = packets.gather(data[b], inf)
                rows, got = packets.gather_fec(par[b], inf, f)
                b1, r1, rc = packets.fec_recover(bodies, counts, rows, got, inf, f)
                lost, rec = lost + int((counts == 0).sum()), rec + int(rc.sum())
                plain.append(packets.unpack_bodies(bodies, counts, inf))
                fixed.append(packets.unpack_bodies(b1, r1, inf))
            share[name] = {"lost": lost, "recovered": rec, "share": rec / lost if lost else None}
            arrays[name] = (plain, fixed)

        def z_of(k):
            ti, tv = zip(*arrays["tactile"][k])
            ai, av = zip(*arrays["audio"][k])
            dv = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x)).to(dev).to(dt)
            return net.decode_latents(dv(np.stack(ai, axis=0), torch.int64), dv(np.stack(ti, axis=1), torch.int64),
                                      nb_valid=dv(np.stack(tv), torch.uint8), na_valid=dv(np.stack(av), torch.uint8))
        per_chunk = lambda x: [float((x[..., s:s + 16] - z_run[..., s:s + 16]).abs().max()) for s in range(0, info.T, 16)]
        out[f"{int(100 * rate)}%"] = {"recovered": share, "drift": {"without_fec": per_chunk(z_of(0)), "with_fec": per_chunk(z_of(1))}}
    return out


KERNELS = ("fec_parity_kernel", "fec_recover_kernel", "fec_rs_parity_kernel", "fec_rs_recover_kernel")


def kernels_and_overhead(net, a, t, fecs, ops, packets):
    """(c) and (d) for one batch and one pair of codes."""
    sent = net.compress_packets_av(a, t, fec=fecs[0], audio_fec=fecs[1])
    ops.profile_begin()
    net.compress_packets_av(a, t, fec=fecs[0], audio_fec=fecs[1])
    net.decompress_packets_av(*sent[:4], fec=fecs[0], fec_packets=sent[4], audio_fec=fecs[1], audio_fec_packets=sent[5])
    prof = ops.profile_end()
    info, ainfo = sent[0][0], sent[2][0]
    return {"kernel_us": {k: 1e6 * prof[k]["seconds"] / prof[k]["launches"] for k in KERNELS if k in prof},
            "overhead_kbps": {
                "tactile": {"bodies": packets.fec_kbps(info, fecs[0], headers=False), "with_headers": packets.fec_kbps(info, fecs[0]),
                            "data_bodies": packets.sent_kbps(info.nb, info, headers=False), "data_with_headers": packets.sent_kbps(info.nb, info)},
                "audio": {"bodies": packets.fec_kbps(ainfo, fecs[1], headers=False), "with_headers": packets.fec_kbps(ainfo, fecs[1]),
                          "data_bodies": packets.sent_kbps(ainfo.nb, ainfo, headers=False), "data_with_headers": packets.sent_kbps(ainfo.nb, ainfo)}}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: the existing paths are also measured on it, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--loss-batch", type=int, default=6)
    ap.add_argument("--parity", default=None, help="extra codes G:R[,G:R...]: Fec(G, 3, R) + Fec(G, 4, R), reported under out['parity']")
    ap.add_argument("--old-only", action="store_true", help="internal: print the existing paths' rows for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    dev = torch.device("cuda:0")
    if args.old_only:
        print(json.dumps({"old": rows_of(_net(dev), args, synth)}))
        return
    from multimodal_vqvae_compression_audio_tactile_amd import ops, packets
    fecs = (packets.Fec(4, 3), packets.Fec(4, 4))
    parent, here = children(args, [args.a_root, ROOT]) if args.a_root else ([], children(args, [ROOT])[0])
    net = _net(dev)
    with_fec = rows_of(net, args, synth, fecs)
    out = {"books": BOOKS, "K": K, "T_lat": 75, "packet_tok": PTOK, "repeats": args.repeats, "warmup": args.warmup,
           "fec": [4, 3], "audio_fec": [4, 4], "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            row = {"B": B, "existing": {}, "fec": with_fec[B]}
            for key in KEYS:
                runs = [h[B][key] for h in here]
                e = {"runs": runs, "spread": max(runs) - min(runs)}
                if parent:
                    pr = [p[B][key] for p in parent]
                    e.update(parent_runs=pr, parent_spread=max(pr) - min(pr), median_minus_parent_median=statistics.median(runs) - statistics.median(pr),
                             ranges_overlap=min(runs) <= max(pr) and min(pr) <= max(runs))
                row["existing"][key] = e
            a, t = synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)
            row.update(kernels_and_overhead(net, a, t, fecs, ops, packets))
            out["rows"].append(row)
        B = args.loss_batch
        a, t = synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)
        out["loss"] = {"B": B, "rates": loss_rows(net, a, t, fecs, (0.05, 0.10, 0.20), 5, packets)}
        if args.parity:                                                   # the same channel seeds: the codes see the same data losses
            out["parity"] = []
            for g, r in ((int(v) for v in spec.split(":")) for spec in args.parity.split(",")):
                f2 = (packets.Fec(g, 3, r), packets.Fec(g, 4, r))
                timed_rows, entry = rows_of(net, args, synth, f2), {"fec": [g, 3, r], "audio_fec": [g, 4, r], "rows": []}
                for Bk in (int(b) for b in args.batches.split(",")):
                    ak, tk = synth.audio_segments(Bk, seed=11).to(dev), synth.tactile_segments(Bk, seed=11).to(dev)
                    entry["rows"].append({"B": Bk, "fec": timed_rows[Bk], **kernels_and_overhead(net, ak, tk, f2, ops, packets)})
                entry["loss"] = {"B": B, "rates": loss_rows(net, a, t, f2, (0.05, 0.10, 0.20), 5, packets)}
                out["parity"].append(entry)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
