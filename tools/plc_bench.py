#!/usr/bin/env python3
"""Packet-loss concealment on the MI355X: one JSON line with
  * the PLC training step at the reference batch of 6 x 1 s (forward_step, TrainingLoss, backward, clip 3.0, AdamW),
  * PLC inference at B = 1 for 1-, 4- and 30-s files (forward_step under no_grad),
  * the time the two full-sequence attention kernels take inside each (the library's per-launch HIP-event profiler, in a
    separate profiled pass so that the timed passes carry no events).
Timing: torch.cuda events around each call after warm-ups, median of the repeats (/opt guides: measuring-on-mi355x).
Seeded synthetic weights and signals (package synth).

  python tools/plc_bench.py [--repeats 10] [--warmup 3]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


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
    return statistics.median(ms), min(ms), max(ms)


def attention_ms(fn):
    """Milliseconds of the attention_seq kernels (forward, backward) in one profiled call of fn."""
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    torch.cuda.synchronize()
    ops.profile_begin()
    try:
        fn()
    finally:
        prof = ops.profile_end()
    fwd = sum(v["seconds"] for k, v in prof.items() if k.startswith("attention_seq_kernel")) * 1e3
    bwd = sum(v["seconds"] for k, v in prof.items() if k.startswith("attention_seq_bwd")) * 1e3
    return fwd, bwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from multimodal_vqvae_compression_audio_tactile_amd import TrainingLoss, build_plc, synth
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
    import plc_inputs as pi
    dev = torch.device("cuda:0")
    net = build_plc(pi.plc_state(), device=dev)
    res = {"metric": "plc", "device": torch.cuda.get_device_name(0), "repeats": args.repeats, "warmup": args.warmup}

    # ---- training step, B = 6 x 1 s
    net.train()
    a, t = synth.audio_segments(6, seed=5, T=24000).to(dev), synth.tactile_segments(6, seed=5, T=24000).to(dev)
    crit = TrainingLoss()
    params = [p for p in net.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=2e-4, weight_decay=1e-5)

    def step():
        opt.zero_grad(set_to_none=True)
        out = net.forward_step(a, t)
        total = crit(out["y_hat"], out["tgt"])
        total.backward()
        torch.nn.utils.clip_grad_norm_(params, 3.0)
        opt.step()
    med, lo, hi = timed(step, args.warmup, args.repeats)
    f, b = attention_ms(step)
    res["train_step_b6_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3),
                               "attention_fwd_ms": round(f, 4), "attention_bwd_ms": round(b, 4),
                               "attention_share": round((f + b) / med, 5)}
    # ---- inference, B = 1
    net.eval()
    for sec in (1, 4, 30):
        a1, t1 = synth.audio_segments(1, seed=6, T=24000 * sec).to(dev), synth.tactile_segments(1, seed=6, T=24000 * sec).to(dev)

        def infer():
            with torch.no_grad():
                net.forward_step(a1, t1)
        med, lo, hi = timed(infer, args.warmup, args.repeats)
        f, _ = attention_ms(infer)
        res[f"infer_b1_{sec}s_ms"] = {"median": round(med, 3), "min": round(lo, 3), "max": round(hi, 3),
                                      "attention_fwd_ms": round(f, 4), "attention_share": round(f / med, 5)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
