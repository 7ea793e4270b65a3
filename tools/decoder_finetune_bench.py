#!/usr/bin/env python3
"""Fine-tuning the tactile decoder on the MI355X: one JSON line with, per batch size B (6 / 256 one-second segments, 8 books x K = 512),
  (a) step_ms      the training step of `bench.py --workload train` (forward_step -> L1 + MRSTFT + MelCos -> backward -> clip + AdamW
                   -> codebook EMA) with the decoder frozen (the reference's configuration) and with train.unfreeze_decoder, and the
                   peak allocated memory of each; with --a-root, a built checkout of the parent commit, the FROZEN step is measured on
                   BOTH trees in fresh child processes, alternating, --a-runs times each: the frozen path has no changed launch, so
                   this tree must sit inside the spread of the parent's own runs (`outside_parent_spread` lists a row that does not);
  (b) layers       per conv of the decoder (k7 and 1x1 of one ResidualUnit per stage, the four transposed convs, model.0 and the
                   final conv): the weight-gradient launch (ops.conv1d_wgrad with Snake staged on load, split-K reduce included) and
                   the forward conv of the same layer in the same run, per launch, with the achieved TFLOP/s of each.  The FLOPs are
                   equal (2 cin cout ks tokens), so the forward is the yardstick.  Reported, not gated.
Timing: torch.cuda events around each call after the warm-ups, median of the repeats; the events bracket host work too.  Seeded
synthetic weights and signals: the times mean something, the losses exercise plumbing only.

  python tools/decoder_finetune_bench.py [--repeats 5] [--warmup 2] [--batches 6,256] [--a-root PATH] [--a-runs 3] [--no-layers]
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


def make_step(mvq, net, a, t):
    """bench.py --workload train's step body."""
    crit = mvq.TrainingLoss()
    params = [p for n, p in net.named_parameters() if p.requires_grad and not n.startswith("vq.books")]
    opt = mvq.optim.AdamW(params, lr=2e-4, weight_decay=1e-5)

    def step():
        with torch.enable_grad():
            out = net.forward_step(a, t)
            total = crit(out["y_hat"], out["tgt"])
            opt.zero_grad(set_to_none=True)
            total.backward()
        _, coef = mvq.optim.clip_coef(params, 3.0)
        opt.step(clip_coef=coef)
        net.vq.ema_step(out["r_tokens"])
    return step


def step_rows(args, trainable):
    """{B: (ms, peak GiB)} of the training step on whatever package sys.path resolves to."""
    import multimodal_vqvae_compression_audio_tactile_amd as mvq
    from multimodal_vqvae_compression_audio_tactile_amd import synth
    dev = torch.device("cuda:0")
    rows = {}
    for B in (int(b) for b in args.batches.split(",")):
        torch.manual_seed(1234)
        net = mvq.build_proposed(synth.proposed_model_state(7, rvq_books=BOOKS, rvq_embed=K), rvq_books=BOOKS, rvq_embed=K, device=dev,
                                 cls=mvq.AllPredAR)
        net.train()
        if trainable:
            from multimodal_vqvae_compression_audio_tactile_amd import train
            train.unfreeze_decoder(net)
        a, t = synth.audio_segments(B, seed=7).to(dev), synth.tactile_segments(B, seed=7).to(dev)
        step = make_step(mvq, net, a, t)
        torch.cuda.reset_peak_memory_stats()
        ms = timed(step, args.warmup, args.repeats)
        rows[B] = (ms, torch.cuda.max_memory_allocated() / 2 ** 30)
        del net, step
        torch.cuda.empty_cache()
    return rows


def child(args, root):
    c = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--frozen-only", "--root", str(root), "--repeats", str(args.repeats),
                        "--warmup", str(args.warmup), "--batches", args.batches], capture_output=True, text=True, timeout=1500)
    if c.returncode != 0:
        raise SystemExit(f"the child on {root} failed:\n" + c.stdout[-2000:] + c.stderr[-2000:])
    return {int(k): v[0] for k, v in json.loads(c.stdout.strip().splitlines()[-1])["frozen"].items()}


def layer_rows(dev, B, args):
    """Weight-gradient launch against the forward conv, layer by layer at the decoder's own lengths (75 latent frames)."""
    from multimodal_vqvae_compression_audio_tactile_amd import Decoder, ops, synth
    dec = Decoder(); dec.load_state_dict(synth.decoder_state(74), strict=True); dec = dec.to(dev)
    m = dec.model
    nblk = len(m) - 4
    layers = [("head k7 1024->1536", "head", m[0], None, 75)]
    t = 75
    for i in range(1, nblk + 1):
        blk = m[i].block
        up = blk[1]
        layers.append((f"transposed {up.cin}->{up.cout} s{up.stride}", "transposed", up, blk[0].flat(), t))
        t = (t - 1) * up.stride - 2 * up.padding + up.ks + up.output_padding
        ru = blk[4].block                                              # the dilation-9 unit: the widest staged window
        layers.append((f"k7 {ru[1].cin} d{ru[1].dilation}", "k7", ru[1], ru[0].flat(), t))
        layers.append((f"1x1 {ru[3].cin}", "1x1", ru[3], ru[2].flat(), t))
    layers.append((f"final k7 {m[nblk + 2].cin}->1", "final", m[nblk + 2], m[nblk + 1].flat(), t))
    g = torch.Generator().manual_seed(B)
    rows = []
    for name, family, conv, alpha, tin in layers:
        x = torch.randn(B, conv.cin, tin, generator=g).to(dev)
        y = conv.run(x, alpha_in=alpha)
        gy = torch.randn(y.shape, generator=g).to(dev)
        flops = 2.0 * conv.cin * conv.cout * conv.ks * B * (tin if family == "transposed" else y.shape[-1])
        n = 5 if B * tin > 100000 else 20
        fwd = timed(lambda: [conv.run(x, alpha_in=alpha) for _ in range(n)], 1, args.repeats) / n
        wg = timed(lambda: [conv.wgrad(gy, x, alpha) for _ in range(n)], 1, args.repeats) / n
        rows.append({"layer": name, "family": family, "tokens": tin, "gflop": flops / 1e9, "forward_us": 1e3 * fwd, "wgrad_us": 1e3 * wg,
                     "forward_tflops": flops / (fwd * 1e-3) / 1e12, "wgrad_tflops": flops / (wg * 1e-3) / 1e12})
        del x, y, gy
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batches", default="6,256")
    ap.add_argument("--a-root", default=None, help="a built checkout of the parent commit: the frozen step is measured on both trees, in child processes")
    ap.add_argument("--a-runs", type=int, default=3)
    ap.add_argument("--no-layers", action="store_true", help="skip the per-layer table")
    ap.add_argument("--frozen-only", action="store_true", help="internal: print the frozen-step rows for the package under --root and exit")
    ap.add_argument("--root", default=str(ROOT))
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.root).resolve()))
    if args.frozen_only:
        print(json.dumps({"frozen": step_rows(args, False)}))
        return
    parent, here = [], []
    for _ in range(args.a_runs if args.a_root else 0):                       # alternating, each run a fresh process
        parent.append(child(args, args.a_root))
        here.append(child(args, ROOT))
    dev = torch.device("cuda:0")
    frozen, trainable = step_rows(args, False), step_rows(args, True)
    out = {"books": BOOKS, "K": K, "T_lat": 75, "repeats": args.repeats, "warmup": args.warmup, "rows": [], "outside_parent_spread": []}
    for B in (int(b) for b in args.batches.split(",")):
        row = {"B": B, "step_ms": {"frozen": frozen[B][0], "trainable": trainable[B][0]},
               "peak_gib": {"frozen": frozen[B][1], "trainable": trainable[B][1]}}
        if parent:
            p, h = [r[B] for r in parent], [r[B] for r in here]
            row["frozen_vs_parent"] = {"parent_runs": p, "this_tree_runs": h, "parent_spread": max(p) - min(p),
                                       "this_tree_median_minus_parent_median": statistics.median(h) - statistics.median(p)}
            if not min(p) <= statistics.median(h) <= max(p):
                out["outside_parent_spread"].append({"B": B, "this_tree_median": statistics.median(h), "parent_min": min(p), "parent_max": max(p)})
        if not args.no_layers:
            row["layers"] = layer_rows(dev, B, args)
        out["rows"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
