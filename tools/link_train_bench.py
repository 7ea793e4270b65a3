#!/usr/bin/env python3
"""The training step under a lossy link on the MI355X: one JSON line with, per batch size B (6 / 256 one-second segments, T_lat = 75,
8 books x K = 512, packets of 2 tokens),
  (a) step_ms        AllPredAR.forward_step -> L1 -> backward (gradients cleared, no optimiser) with link=None (the default step) and
                     under a packets.Link (a burst channel on each stream) in the three audio_conceal modes; with --a-root, a built
                     checkout of the parent commit, the link=None step is measured on BOTH trees in fresh child processes,
                     alternating, --a-runs times each: the spread of the parent's runs is the margin within which the default step
                     did not move;
  (b) plc_step_ms    AllPredPLC.forward_step -> L1 -> backward, default and na_valid= with "mask" / "hold";
  (c) kernel_us      the masked attention backward against the plain one, per launch: the chunk form in the step's folded layout
                     (B items, 16 queries x 16 keys) and the sequence form at Tq = Tk = 75, about a quarter of the keys absent;
  (d) draw_us        ops.channel_draw per launch.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  Seeded
synthetic weights and signals: the times mean something, the losses exercise plumbing only.

  python tools/link_train_bench.py [--repeats 5] [--warmup 2] [--batches 6,256] [--a-root PATH] [--a-runs 3]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
BOOKS, K, PTOK = 8, 512, 2


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


def train_step(net, a, t, **kw):
    def step():
        with torch.enable_grad():
            out = net.forward_step(a, t, **kw)
            (out["y_hat"] - out["tgt"]).abs().mean().backward()
        for p in net.parameters():
            p.grad = None
    return step


def default_rows(args):
    """The link=None step on whatever package sys.path resolves to."""
    from multimodal_vqvae_compression_audio_tactile_amd import AllPredAR, build_proposed, synth
    dev = torch.device("cuda:0")
    net = build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev, cls=AllPredAR)
    rows = {}
    for B in (int(b) for b in args.batches.split(",")):
        a, t = synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)
        rows[B] = timed(train_step(net, a, t), args.warmup, args.repeats)
    return rows


def child(args, root):
    c = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--default-only", "--root", str(root), "--repeats", str(args.repeats),
                        "--warmup", str(args.warmup), "--batches", args.batches], capture_output=True, text=True, timeout=900)
    if c.returncode != 0:
        raise SystemExit(f"the child on {root} failed:\n" + c.stdout[-2000:] + c.stderr[-2000:])
    return {int(k): v for k, v in json.loads(c.stdout.strip().splitlines()[-1])["default"].items()}


def kernel_rows(dev, B, repeats):
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    H, dh = 8, 128
    g = torch.Generator().manual_seed(B)
    rows = {}
    for form, T in (("chunk", 16), ("seq", 75)):
        q, k, v, go = (torch.randn(1, H * dh, B * T, generator=g).to(dev) for _ in range(4))
        mask = (torch.rand(B, T, generator=g) < 0.75).to(torch.uint8).to(dev)
        bwd = ops.attention_bwd if form == "chunk" else ops.attention_seq_bwd
        n = 20
        plain = timed(lambda: [bwd(q, k, v, go, H, folded_batch=B) for _ in range(n)], 2, repeats)
        masked = timed(lambda: [bwd(q, k, v, go, H, folded_batch=B, kmask=mask) for _ in range(n)], 2, repeats)
        rows[form] = {"T": T, "plain_us": 1e3 * plain / n, "masked_us": 1e3 * masked / n}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: the link=None step is measured on both trees, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--default-only", action="store_true", help="internal: print the link=None rows for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.default_only:
        print(json.dumps({"default": default_rows(args)}))
        return
    parent, here = [], []
    for _ in range(args.a_runs if args.a_root else 0):                       # alternating, each run a fresh process
        parent.append(child(args, args.a_root))
        here.append(child(args, ROOT))
    from multimodal_vqvae_compression_audio_tactile_amd import AllPredAR, build_plc, build_proposed, ops, packets, synth
    dev = torch.device("cuda:0")
    sd = synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K)
    net = build_proposed(sd, rvq_books=BOOKS, rvq_embed=K, device=dev, cls=AllPredAR)
    plc = build_plc(device=dev)
    plc.load_state_dict({k: v for k, v in sd.items() if k.split(".")[0] in ("A_ENC", "A_QUANT", "T_ENC", "T_DEC", "predict", "tokennorm")}, strict=False)
    burst = dict(loss=0.02, thin=0.3, p_gb=0.05, p_bg=0.3, loss_bad=0.8)
    link = packets.Link(packets.Channel(seed=1, **burst), packets.Channel(seed=2, **burst), PTOK)
    out = {"books": BOOKS, "K": K, "T_lat": 75, "packet_tok": PTOK, "repeats": args.repeats, "warmup": args.warmup, "channel": burst, "rows": []}
    for B in (int(b) for b in args.batches.split(",")):
        a, t = synth.audio_segments(B, seed=11).to(dev), synth.tactile_segments(B, seed=11).to(dev)
        row = {"B": B, "step_ms": {"default": timed(train_step(net, a, t), args.warmup, args.repeats)}}
        for mode in ("zero", "mask", "hold"):
            row["step_ms"]["link_" + mode] = timed(train_step(net, a, t, link=link, step=3, audio_conceal=mode), args.warmup, args.repeats)
        if parent:
            p, h = [r[B] for r in parent], [r[B] for r in here]
            row["default_vs_parent"] = {"parent_runs": p, "this_tree_runs": h, "parent_spread": max(p) - min(p),
                                        "this_tree_median_minus_parent_median": statistics.median(h) - statistics.median(p)}
        nav = ops.channel_draw(link.audio, 32, 75, PTOK, B, stream=1, step=3, device=dev)
        row["plc_step_ms"] = {"default": timed(train_step(plc, a, t), args.warmup, args.repeats)}
        for mode in ("mask", "hold"):
            row["plc_step_ms"][mode] = timed(train_step(plc, a, t, na_valid=nav, audio_conceal=mode), args.warmup, args.repeats)
        row["kernel_us"] = kernel_rows(dev, B, args.repeats)
        n = 50
        row["draw_us"] = 1e3 * timed(lambda: [ops.channel_draw(link.tactile, BOOKS, 75, PTOK, B, step=i, device=dev) for i in range(n)], 2,
                                     args.repeats) / n
        with torch.no_grad():                                                  # nothing lost: the receiver-order sum against the default step
            base = net.forward_step(a, t)["y_hat"]
            full = net.forward_step(a, t, nb_valid=torch.full((B, 75), BOOKS, dtype=torch.uint8, device=dev))["y_hat"]
            row["nothing_lost_rel_l2_vs_default"] = float((full - base).double().norm() / base.double().norm())
            o = net.forward_step(a, t, link=link, step=3)
            row["lost_fraction"] = {"tactile": float((o["nb_valid"] == 0).float().mean()), "audio": float((o["na_valid"] == 0).float().mean())}
        out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
