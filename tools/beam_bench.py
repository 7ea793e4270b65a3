#!/usr/bin/env python3
"""The sender's beam search over the books on the MI355X: one JSON line with
  (a) quality     on the tokens the sender's search sees (the r_tokens of the closed loop on seeded weights, synth.proposed_model_state,
                  over the synthetic corpus) and on plain Gaussian tokens and books: per beam in {2, 4, 8}
                  gain_db = 10 log10(sum E_nb greedy / sum E_nb beam), the per-prefix curves mean E_m of both paths (the beam optimises
                  the full depth: its prefixes may be worse), and the share of tokens where a non-greedy slot won;
  (b) launch_us   per batch size B the beam launch's time per 16-token chunk from the library's profile events (rvq_beam_kernel), next
                  to the greedy launch's (torch.cuda events around ops.rvq_ema_forward on the same chunk: it records no profile event);
  (c) compress_packets_ms / step_ms   the whole-item sender and the StreamSender steady step (a 16-token push) with rate=None, Rate()
                  and Rate(beam=4); with --a-root, a built checkout of the parent commit, the rate=None and Rate() rows are measured in
                  fresh child processes on both trees alternating, --a-runs times each: no new code runs there, so this tree is
                  expected inside the parent's own spread.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  Seeded
synthetic weights and signals: the times mean something, the gain exercises plumbing only (untrained books).

  python tools/beam_bench.py [--repeats 10] [--warmup 3] [--batches 1,6,256] [--corpus 64] [--a-root PATH] [--a-runs 3]
"""
import argparse
import json
import math
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K, PTOK, D = 8, 512, 2, 96
STEP = 5120
BEAMS = (2, 4, 8)


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


def steady_push(net, a, t, B, **kw):
    """A session in its steady state -> the function that pushes its next 16 tokens (the 1-s signal repeats)."""
    tx = net.stream_sender(batch=B, **kw)
    n_steps, state = a.shape[-1] // STEP, {"c": 0}

    def push():
        c = state["c"] % n_steps
        state["c"] += 1
        return tx.push(a[..., STEP * c:STEP * (c + 1)], t[..., STEP * c:STEP * (c + 1)])
    push(), push(), push()
    return push


def model(dev):
    from multimodal_vqvae_compression_audio_tactile_amd import build_proposed, synth
    return build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev)


def beam_off_rows(args):
    """rate=None and Rate() -- the paths no new code runs on -- on whatever package sys.path resolves to."""
    from multimodal_vqvae_compression_audio_tactile_amd import packets, synth
    dev = torch.device("cuda:0")
    net = model(dev)
    rows = {}
    with torch.no_grad():
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            rows[B] = {}
            for name, kw in (("none", {}), ("rate", {"rate": packets.Rate()})):
                rows[B][name] = {"compress_packets_ms": timed(lambda: net.compress_packets(a, t, **kw), args.warmup, args.repeats),
                                 "step_ms": timed(steady_push(net, a, t, B, **kw), args.warmup, args.repeats)}
    return rows


def quality(ops, packets, z, books):
    """z[B, 96, T] and books[nb, K, 96] on the device -> the figures of (a)."""
    nb, n = books.shape[0], z.shape[0] * z.shape[2]
    _, g_idx = ops.rvq_ema_forward(z, books, return_indices="int32")
    g_E = ops.rvq_rate(z, g_idx, books, packets.Rate(), 1, want_energy=True)[3].double()
    out = {"tokens": n, "greedy_mean_E_m": g_E.mean(dim=1).tolist()}
    for beam in BEAMS:
        idx, slot = ops.rvq_beam(z, books, beam, want_slot=True)
        E = ops.rvq_rate(z, idx, books, packets.Rate(), 1, want_energy=True)[3].double()
        assert bool((E[nb] <= g_E[nb]).all())
        out[f"beam{beam}"] = {"gain_db": 10.0 * math.log10(float(g_E[nb].sum()) / float(E[nb].sum())),
                              "mean_E_m": E.mean(dim=1).tolist(),
                              "prefix_gain_db": [10.0 * math.log10(float(g_E[m].sum()) / float(E[m].sum())) for m in range(1, nb + 1)],
                              "non_greedy_share": float((slot != 0).double().mean()),
                              "tokens_strictly_better": int((E[nb] < g_E[nb]).sum())}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,6,256")
    ap.add_argument("--corpus", type=int, default=64, help="one-second segments of the synthetic corpus the quality figures run over")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: rate=None and Rate() are measured on both trees")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--off-only", action="store_true", help="internal: print the rate=None / Rate() rows for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.off_only:
        print(json.dumps({"off": beam_off_rows(args)}))
        return

    def child(root):
        c = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--off-only", "--root", str(root), "--repeats", str(args.repeats),
                            "--warmup", str(args.warmup), "--batches", args.batches], capture_output=True, text=True, timeout=900)
        if c.returncode != 0:
            raise SystemExit(f"the child on {root} failed:\n" + c.stdout[-2000:] + c.stderr[-2000:])
        return {int(k): v for k, v in json.loads(c.stdout.strip().splitlines()[-1])["off"].items()}
    parent, here = [], []
    for _ in range(args.a_runs if args.a_root else 0):                    # the two trees alternating, each in a fresh process
        parent.append(child(args.a_root))
        here.append(child(ROOT))
        print(f"beam_bench: A/B pass {len(here)} of {args.a_runs} done", file=sys.stderr, flush=True)

    from multimodal_vqvae_compression_audio_tactile_amd import ops, packets, synth
    dev = torch.device("cuda:0")
    net = model(dev)
    out = {"books": BOOKS, "K": K, "T_lat": 75, "packet_tok": PTOK, "repeats": args.repeats, "warmup": args.warmup, "rows": []}
    with torch.no_grad():
        # (a) the tokens the search sees in the closed loop (greedy history), then Gaussian tokens against Gaussian books
        a, t = inputs(args.corpus, dev, synth)
        codes = net.A_QUANT(net.A_ENC(a))[1]
        r_tokens = net._ar_latents(net.A_QUANT.from_codes(codes)[0], net.T_ENC(t), want_tokens=True, rate=packets.Rate())[1]
        books = net.vq.stacked()
        out["quality_seeded_head"] = quality(ops, packets, r_tokens, books)
        g = torch.Generator(device="cpu").manual_seed(5)
        zg = torch.randn(args.corpus, D, 75, generator=g).to(dev)
        # book m: N(0, (0.36 * 0.93^m)^2) -- the best of 512 random directions in 96 dimensions has a cosine near sqrt(2 ln K / D) = 0.36,
        # so a code of that relative length removes about 13 % of the residual energy, and the next book is scaled to what is left
        bg = torch.stack([torch.randn(K, D, generator=g) * (0.36 * 0.93 ** m) for m in range(BOOKS)]).to(dev)
        out["quality_gaussian"] = quality(ops, packets, zg, bg)
        for B in (int(b) for b in args.batches.split(",")):
            a, t = inputs(B, dev, synth)
            row = {"B": B}
            # (b) one chunk of B * 16 tokens, token-folded as the loop hands it over
            zc = r_tokens[:1].expand(B, -1, -1)[..., :16].permute(1, 0, 2).reshape(1, D, B * 16).contiguous()
            row["launch_us"] = {"greedy_events": 1e3 * timed(lambda: ops.rvq_ema_forward(zc, books, return_indices="int32"), args.warmup, args.repeats),
                                "greedy_kernel": ops.rvq_ema_forward_kernel_name(1, D, B * 16, K)}
            for beam in BEAMS:
                for _ in range(args.warmup):
                    ops.rvq_beam(zc, books, beam, folded_batch=B)
                ops.profile_begin()
                for _ in range(args.repeats):
                    ops.rvq_beam(zc, books, beam, folded_batch=B)
                prof = ops.profile_end()["rvq_beam_kernel"]
                row["launch_us"][f"beam{beam}"] = 1e6 * prof["seconds"] / prof["launches"]
            # (c) the surfaces
            for name, kw in (("none", {}), ("rate", {"rate": packets.Rate()}), ("beam4", {"rate": packets.Rate(beam=4)})):
                row[name] = {"compress_packets_ms": timed(lambda: net.compress_packets(a, t, **kw), args.warmup, args.repeats),
                             "step_ms": timed(steady_push(net, a, t, B, **kw), args.warmup, args.repeats)}
            if parent:
                for name in ("none", "rate"):
                    for key in ("compress_packets_ms", "step_ms"):
                        p, h = [r[B][name][key] for r in parent], [r[B][name][key] for r in here]
                        row[name]["ab_" + key] = {"parent_runs": p, "this_tree_runs": h, "parent_spread": max(p) - min(p),
                                                  "this_tree_median_minus_parent_median": statistics.median(h) - statistics.median(p),
                                                  "inside_parent_spread": min(p) <= statistics.median(h) <= max(p)}
            out["rows"].append(row)
            print(f"beam_bench: B = {B} done", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
