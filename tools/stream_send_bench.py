#!/usr/bin/env python3
"""The streaming sender on the MI355X: one JSON line with, per batch size B (1 / 6 / 256 sessions in lockstep, 8 books x K = 512,
packets of 2 tokens),
  (a) step_eager_ms / step_graph_ms   one steady push (16 new tokens onto the 24 held ones of a session fed 16 tokens at a time, the
                                      32-token encoder window, 16 tokens of packets and audio codes out), run eagerly and as the replayed graph
                                      (StreamSender(graph=True)), host work included;
  (b) split                           the eager step taken apart, each stage alone: the upload of the 2 x 5120 new samples, the
                                      sample-state kernel, A_ENC and T_ENC on the window (each alone on one stream; the step
                                      itself overlaps them on two streams up to 64 sessions), A_QUANT on the 16 tokens, the AR
                                      chunk with the carried token, and pack + the one device-to-host copy + framing;
  (c) real_time_factor                step time / 213.3 ms (the signal a chunk carries);
  (d) latency_ms                      320 ms (one chunk + the 8-token encoder look-ahead) + the step time;
  (e) whole_item_ms                   compress_packets on a whole 75-token item, of this tree and -- with --a-root, a built
                                      checkout of the parent commit, in fresh child processes -- of the parent, --a-runs times:
                                      the spread of those runs is the margin within which the whole-item path did not move.
  (f) --encoder stateful|both         rows for StreamSender(encoder="stateful") beside the window mode's, in ONE process: the steady
                                      step (16 new tokens fed to the stateful encoders, nothing encoded twice) eagerly and as the
                                      graph, and "encode_ms": the two encoders of a steady step alone, window against stateful,
                                      --rounds times alternating (the window rows' max - min is the spread the stateful row must
                                      beat).  The stateful encode restores its state before every call; the restore is timed
                                      alone and subtracted.  With --a-root the parent's window-mode step is measured too, parent
                                      and this tree alternating.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  A steady
step is timed on a session that keeps running (every timed push is a real next chunk of a signal that repeats).  Seeded synthetic
weights and signals: only the times mean anything.  The only threshold enforced is the format's own: one session (B = 1) must
take less than the 213.3 ms of signal a step carries.

  python tools/stream_send_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--a-root PATH] [--a-runs 3]
                                    [--encoder window|stateful|both] [--rounds 3]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K = 8, 512
CHUNK_MS, LOOKAHEAD_MS = 16 / 75 * 1000.0, 8 / 75 * 1000.0
STEP = 5120                                                               # samples of a steady push


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


def steady_session(net, a, t, B, graph, encoder="window"):
    """A session in its steady state -> (tx, push): three pushes of 16 tokens have run (nothing, chunk 0, the first steady step)."""
    n_steps = a.shape[-1] // STEP                                             # the 1-s signal repeats every four pushes
    tx = net.stream_sender(batch=B, graph=graph) if encoder == "window" else net.stream_sender(batch=B, graph=graph, encoder=encoder)
    state = {"c": 0}

    def push():
        c = state["c"] % n_steps
        state["c"] += 1
        return tx.push(a[..., STEP * c:STEP * (c + 1)], t[..., STEP * c:STEP * (c + 1)])
    push(), push(), push()
    return tx, push


def whole_item_rows(args, net=None):
    """(e), and the window-mode steady step, on whatever package sys.path resolves to."""
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    dev = torch.device("cuda:0")
    if net is None:
        net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    rows, steps = {}, {}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            rows[B] = timed(lambda: net.compress_packets(a, t), args.warmup, args.repeats)
            steps[B] = [timed(steady_session(net, a, t, B, graph)[1], args.warmup, args.repeats) for graph in (False, True)]
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
    ap.add_argument("--encoder", default="window", choices=("window", "stateful", "both"))
    ap.add_argument("--rounds", type=int, default=3, help="alternating rounds of the encode stage, window against stateful")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.whole_only:
        whole, steps = whole_item_rows(args)
        print(json.dumps({"whole": whole, "step": steps}))
        return
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, ops, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)
    parent, parent_step, here_runs, here_step = [], [], [], []
    for _ in range(args.a_runs if args.a_root else 0):
        child = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--whole-only", "--root", args.a_root, "--repeats",
                                str(args.repeats), "--warmup", str(args.warmup), "--batches", args.batches],
                               capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            raise SystemExit("the parent side failed:\n" + child.stdout[-2000:] + child.stderr[-2000:])
        got = json.loads(child.stdout.strip().splitlines()[-1])
        parent.append({int(k): v for k, v in got["whole"].items()})
        parent_step.append({int(k): v for k, v in got.get("step", {}).items()})
        w, st = whole_item_rows(args, net)                                    # parent and this tree alternating
        here_runs.append(w)
        here_step.append(st)
    here = whole_item_rows(args, net)[0]
    out = {"books": BOOKS, "K": K, "packet_tok": 2, "chunk_tok": 16, "window_tok": 32, "repeats": args.repeats, "warmup": args.warmup,
           "chunk_ms": CHUNK_MS, "lookahead_ms": LOOKAHEAD_MS, "rows": []}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)

            def session(graph, encoder="window"):
                return steady_session(net, a, t, B, graph, encoder)

            row = {"B": B}
            for name, graph in (("step_eager_ms", False), ("step_graph_ms", True)):
                _, push = session(graph)
                row[name] = timed(push, args.warmup, args.repeats)
            # the eager step's stages, each alone, on a session in its steady state
            tx, _ = session(False)
            fill = tx.fill
            assert (fill, tx.start, tx.chunk) == (24 * 320, 24, 2)
            a_new, t_new = a[..., :STEP], t[..., :STEP]
            x = tx._upload(a_new, t_new, STEP)
            keep = tx.buf.clone()

            def samples():
                tx.buf.copy_(keep)
                return ops.stream_samples(tx.buf, fill, x, 2 * STEP, STEP)
            win = samples()
            a_w, t_w = win[:B].unsqueeze(1), win[B:].unsqueeze(1)
            za = net.A_ENC(a_w)[..., 8:24].contiguous()
            zt = net.T_ENC(t_w)[..., 8:24].contiguous()
            qa = net.A_QUANT(za)[0]
            carry = torch.zeros(B, tx.C, device=dev)
            idx = net._ar_latents(qa, zt, None, want_indices=True, z_prev=carry, z_last_out=carry)[2]

            def pack_out():
                tx.chunk = 2
                return tx._framed(tx._back.pack(idx, None), None, 16)
            restore_ms = timed(lambda: tx.buf.copy_(keep), args.warmup, args.repeats)
            row["split"] = {"upload_ms": timed(lambda: tx._upload(a_new, t_new, STEP), args.warmup, args.repeats),
                            "samples_kernel_ms": max(0.0, timed(samples, args.warmup, args.repeats) - restore_ms),
                            "a_enc_ms": timed(lambda: net.A_ENC(a_w), args.warmup, args.repeats),
                            "t_enc_ms": timed(lambda: net.T_ENC(t_w), args.warmup, args.repeats),
                            "a_quant_ms": timed(lambda: net.A_QUANT(za), args.warmup, args.repeats),
                            "ar_chunk_ms": timed(lambda: net._ar_latents(qa, zt, None, want_indices=True, z_prev=carry, z_last_out=carry),
                                                 args.warmup, args.repeats),
                            "pack_readback_frame_ms": timed(pack_out, args.warmup, args.repeats)}
            for name in ("step_eager_ms", "step_graph_ms"):
                row[name.replace("_ms", "_real_time_factor")] = row[name] / CHUNK_MS
                row[name.replace("step_", "latency_")] = CHUNK_MS + LOOKAHEAD_MS + row[name]
            if args.encoder != "window":
                for name, graph in (("stateful_step_eager_ms", False), ("stateful_step_graph_ms", True)):
                    row[name] = timed(session(graph, "stateful")[1], args.warmup, args.repeats)
                # the encode stage of a steady step alone: window (two 32-token encodes) against stateful (16 new tokens, state
                # restored before every call, the restore timed alone and subtracted), alternating
                txs, _ = session(False, "stateful")
                assert (txs.fill, txs.start, txs.chunk) == (8 * 320, 40, 2)
                keep_s = [s.clone() for s in txs.enc_state]
                a16, t16 = a[:, :, :STEP].contiguous(), t[:, :, :STEP].contiguous()
                before = 320 * txs.start

                def restore():
                    for s, k in zip(txs.enc_state, keep_s):
                        s.copy_(k)

                def enc_stateful():
                    restore()
                    net.A_ENC.forward_stream(txs.enc_state[0], a16, before, False)
                    return net.T_ENC.forward_stream(txs.enc_state[1], t16, before, False)

                def enc_window():
                    net.A_ENC(a_w)
                    return net.T_ENC(t_w)
                rounds = {"window": [], "stateful": []}
                for _ in range(args.rounds):
                    rounds["window"].append(timed(enc_window, args.warmup, args.repeats))
                    rs = timed(restore, args.warmup, args.repeats)
                    rounds["stateful"].append(max(0.0, timed(enc_stateful, args.warmup, args.repeats) - rs))
                row["encode_ms"] = rounds
                row["encode_window_spread_ms"] = max(rounds["window"]) - min(rounds["window"])
                row["encode_ratio"] = statistics.median(rounds["window"]) / max(statistics.median(rounds["stateful"]), 1e-9)
                row["state_bytes_per_session"] = 4 * sum(int(s.shape[1]) for s in txs.enc_state)
            if parent_step and parent_step[0]:
                row["window_step_ms"] = {"parent_runs": [p[B] for p in parent_step], "this_tree_runs": [p[B] for p in here_step]}
            row["whole_item_ms"] = {"this_tree": here[B], "parent_runs": [p[B] for p in parent], "this_tree_runs": [p[B] for p in here_runs]}
            if parent:
                runs = row["whole_item_ms"]["parent_runs"]
                row["whole_item_ms"]["parent_spread"] = max(runs) - min(runs)
                row["whole_item_ms"]["this_tree_minus_parent_median"] = here[B] - statistics.median(runs)
            out["rows"].append(row)
    print(json.dumps(out))
    if any(r["B"] == 1 and min(r["step_eager_ms"], r["step_graph_ms"]) >= CHUNK_MS for r in out["rows"]):
        raise SystemExit("one session does not keep up with real time: the B = 1 step takes longer than the 213.3 ms chunk it encodes")


if __name__ == "__main__":
    main()
