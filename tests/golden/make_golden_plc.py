#!/usr/bin/env python3
"""Generate the packet-loss-concealment fixtures tests/golden/g13..g16 from the REFERENCE's own PLC scripts (run in the build
container only; the reference is not on the GPU machines).

  python tests/golden/make_golden_plc.py

PLC/PLC1.py and PLC/PLC1_eval.py are imported through oracle/ref_import.load (stand-ins for dac / torchaudio / soundfile), the
DAC backbones are the torch restatement oracle/dac24_torch.py (as for G4 / G7), inputs come from seeds (tests/plc_inputs.py):
  G13 AllPredPLC.forward_step (PLC1_eval.py), eval mode: B = 2 x 1 s (T_lat = 75) and B = 1 x 3 s (T_lat = 225) with the mask the
      reference's make_token_loss_mask draws on the seeded CPU generator; stored: that mask, z_pred (flat[::13]), y_hat.  Also the
      CrossPredictor alone at T = 75 and 300 (flat[::13]).
  G14 one PLC1.py training step, B = 2 x 1 s, fixed mask, dropout off (eval mode), fp32, no autocast: the loss parts
      (safe_l1 0.55, MultiResSTFTLoss 0.25, MelCosineLoss 0.20; torchaudio's MelScale replaced by oracle/losses_torch.MelScale),
      the norm and flat[::997] of every predict.* gradient, and the same step in float64 (the reference's model in double,
      losses from oracle/losses_torch, since the reference's loss classes cast to float32), as G7 does.
  G15 mae_subset / snr_subset_db / psnr_subset_db of PLC1_eval.py with its token -> sample mask mapping, including empty subsets.
  G16 AllPredPLC.state_dict() names and shapes (JSON).
Only arrays (G16: names and shapes) are stored, never reference source.
"""
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import plc_inputs as pi                         # noqa: E402
from oracle import dac24_torch as T             # noqa: E402
from oracle import losses_torch as LT           # noqa: E402
from oracle import ref_import                   # noqa: E402

OUT = Path(__file__).resolve().parent
torch.set_grad_enabled(False)


def model(mod, sd, double=False):
    da, dt = T.DAC(), T.DAC()
    net = mod.AllPredPLC(da.encoder, da.quantizer, dt.encoder, dt.decoder, c_lat=1024)
    net.load_state_dict(sd, strict=True)
    net = net.double() if double else net
    return net.eval()


class FixedMask:
    """Replace the module's make_token_loss_mask by one returning `mask` (the training-step fixture uses a fixed mask)."""

    def __init__(self, mod, mask):
        self.mod, self.mask, self.orig = mod, mask, mod.make_token_loss_mask

    def __enter__(self):
        self.mod.make_token_loss_mask = lambda batch_size, T_lat, packet_tok, p_loss, device: self.mask.to(device)

    def __exit__(self, *a):
        self.mod.make_token_loss_mask = self.orig


class Capture:
    """Record what the model's predictor returns (z_pred) while active."""

    def __init__(self, net):
        self.net, self.out = net, []

    def __enter__(self):
        h = self.net.predict.register_forward_hook(lambda m, i, o: self.out.append(o.detach().clone()))
        self.h = h
        return self

    def __exit__(self, *a):
        self.h.remove()


def main():
    assert ref_import.available(), "reference not mounted"
    plc = ref_import.load("PLC/PLC1.py", "ref_plc1")
    ev = ref_import.load("PLC/PLC1_eval.py", "ref_plc1_eval")
    sd = pi.plc_state()

    # ---- G16: state-dict layout
    net = model(plc, sd)
    (OUT / "g16_plc_state_shapes.json").write_text(json.dumps({k: list(v.shape) for k, v in net.state_dict().items()}))

    # ---- G13: forward (eval) + predictor alone
    g13 = {}
    net = model(ev, sd)
    for name, (B, Tw, seed) in pi.FWD_CASES.items():
        a, t = pi.waves(B, Tw, seed)
        torch.manual_seed(pi.MASK_SEED + seed)
        with Capture(net) as cap:
            out = net.forward_step(a, t)
        g13[f"{name}.mask"] = out["latent_mask"][:, 0].numpy()
        g13[f"{name}.z_pred"] = cap.out[0].reshape(-1)[::pi.LAT_STRIDE].numpy().copy()
        g13[f"{name}.y_hat"] = out["y_hat"].numpy()
    cp = net.predict
    for name, (B, Tt, seed) in pi.PRED_CASES.items():
        zt, qa = pi.pred_inputs(B, Tt, seed)
        g13[f"pred.{name}"] = cp(torch.from_numpy(zt), torch.from_numpy(qa)).reshape(-1)[::pi.LAT_STRIDE].numpy().copy()
    np.savez_compressed(OUT / "g13_plc_forward.npz", **g13)

    # ---- G14: one training step (fp32 reference) and the same step in float64
    B, Tw, seed = pi.TRAIN_CASE
    a, t = pi.waves(B, Tw, seed)
    torch.manual_seed(pi.MASK_SEED + seed)
    mask = plc.make_token_loss_mask(B, Tw // 320, plc.PACKET_TOK, plc.PACKET_LOSS_PROB, "cpu")
    g14 = {"mask": mask.numpy()}
    with torch.enable_grad():
        net = model(plc, sd)
        mr, mc = plc.MultiResSTFTLoss(), plc.MelCosineLoss()
        mc.mel = LT.MelScale(n_mels=64, sample_rate=24000, n_stft=257, f_min=0.0, f_max=12000.0)
        with FixedMask(plc, mask):
            out = net.forward_step(a, t)
        assert torch.equal(out["latent_mask"][:, 0], mask)
        y = out["y_hat"]; y.retain_grad()
        l1, st, me = plc.safe_l1(y, out["tgt"]), mr(y, out["tgt"]), mc(y, out["tgt"])
        total = plc.W_WAV_L1 * l1 + plc.W_STFT * st + plc.W_MELCOS * me
        total.backward()
    g14["losses"] = np.array([float(l1), float(st), float(me), float(total)], np.float64)
    g14["y_hat"] = y.detach().numpy()
    for name, p_ in net.named_parameters():
        if p_.grad is not None:
            assert name.startswith("predict."), name
            g14[f"norm.{name}"] = np.array(float(p_.grad.norm()), np.float64)
            g14[f"sub.{name}"] = p_.grad.reshape(-1)[::pi.GRAD_STRIDE].numpy().copy()
    assert net.tokennorm.ln.weight.grad is None
    with torch.enable_grad():
        n64 = model(plc, sd, double=True)
        with FixedMask(plc, mask):
            o64 = n64.forward_step(a.double(), t.double())
        assert (o64["y_hat"] - y.detach().double()).abs().max() < 1e-4
        y64 = o64["y_hat"]
        tot64, (l1_64, st_64, me_64) = LT.total_loss(y64, o64["tgt"])
        tot64.backward()
    g14["f64.losses"] = np.array([float(l1_64), float(st_64), float(me_64), float(tot64)], np.float64)
    for name, p_ in n64.named_parameters():
        if p_.grad is not None:
            g14[f"f64.norm.{name}"] = np.array(float(p_.grad.norm()), np.float64)
            g14[f"f64.sub.{name}"] = p_.grad.reshape(-1)[::pi.GRAD_STRIDE].numpy().copy()
    np.savez_compressed(OUT / "g14_plc_train_step.npz", **g14)

    # ---- G15: subset metrics with the token -> sample mapping of PLC1_eval.py
    ref, est, masks = pi.metric_inputs()
    g15 = {}
    r_, e_ = torch.from_numpy(ref), torch.from_numpy(est)
    for name, lm in masks.items():
        T_wave, T_lat = ref.size, lm.size
        spt = float(T_wave) / float(T_lat)
        tok = torch.clamp(torch.floor(torch.arange(T_wave, dtype=torch.float32) / spt).long(), 0, T_lat - 1)
        sm = torch.from_numpy(lm)[tok]
        g15[f"{name}.sample_mask"] = sm.numpy()
        g15[f"{name}.values"] = np.array([
            ev.mae_subset(r_, e_, sm), ev.mae_subset(r_, e_, ~sm),
            ev.snr_subset_db(r_, e_, sm), ev.snr_subset_db(r_, e_, ~sm),
            ev.psnr_subset_db(r_, e_, sm, pi.METRIC_PEAK), ev.psnr_subset_db(r_, e_, ~sm, pi.METRIC_PEAK)], np.float64)
    np.savez_compressed(OUT / "g15_plc_metrics.npz", **g15)
    for f in ("g13_plc_forward.npz", "g14_plc_train_step.npz", "g15_plc_metrics.npz", "g16_plc_state_shapes.json"):
        print(f, (OUT / f).stat().st_size)


if __name__ == "__main__":
    main()
