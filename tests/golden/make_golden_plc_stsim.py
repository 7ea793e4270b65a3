#!/usr/bin/env python3
"""Generate the PLC evaluation fixtures tests/golden/g17, g18 from the REFERENCE's own evaluation scripts (run in the build
container only; the reference is not on the GPU machines).

  python tests/golden/make_golden_plc_stsim.py

PLC/PLC1_eval.py and PLC/PLC1_low_mid_high_eval.py are imported through oracle/ref_import.load; torchaudio's MelScale is
replaced by oracle/losses_torch.MelScale (as for G7 / G14).  scikit-image is not installed, so the SSIM branch runs with the
module's ``ssim`` replaced by the float32 restatement tests/plc_ref/ssim_ref.py and SKIMAGE_AVAILABLE = True; the norm branch
is the reference as it stands without scikit-image (SKIMAGE_AVAILABLE = False).  Inputs come from tests/plc_eval_inputs.py:
  G17 per case of STSIM_CASES: the frame mask (the reference's float64 token rule), the normalised mel images X, Y of
      _mel_mag, compute_stsim_mel_with_mask in both branches and compute_stsim_mel_global (category script) in both.
  G18 pass-1 rows of eval_model (PLC1_eval.py:601-663) for the two EVAL_FILES at 24 kHz (resample_to is the identity): the
      reference's AllPredPLC with the oracle DAC backbones (tests/plc_inputs.plc_state), the mask fixed to the stored one,
      the reference's helpers in the reference's order, both ST-SIM branches, and mae_global.
Only arrays are stored, never reference source.
"""
import sys
import types
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import plc_eval_inputs as pe                   # noqa: E402
import plc_inputs as pi                        # noqa: E402
from plc_ref import ssim_ref                   # noqa: E402
from oracle import dac24_torch as T            # noqa: E402
from oracle import losses_torch as LT          # noqa: E402
from oracle import ref_import                  # noqa: E402

OUT = Path(__file__).resolve().parent
torch.set_grad_enabled(False)
ROW = ("len_samples", "psnr_global_db", "stsim_global", "psnr_masked_db", "psnr_unmasked_db", "snr_masked_db",
       "snr_unmasked_db", "mae_masked", "mae_unmasked", "stsim_masked", "stsim_unmasked")


def patch(mod):
    mod.torchaudio = types.SimpleNamespace(transforms=types.SimpleNamespace(MelScale=LT.MelScale))
    mod._MEL_CACHE.clear()
    mod.ssim = ssim_ref.ssim_f32
    return mod


class Branch:
    def __init__(self, mods, skimage):
        self.mods, self.skimage = mods, skimage

    def __enter__(self):
        for m in self.mods:
            m.SKIMAGE_AVAILABLE = self.skimage

    def __exit__(self, *a):
        pass


def main():
    assert ref_import.available(), "reference not mounted"
    ev = patch(ref_import.load("PLC/PLC1_eval.py", "ref_plc1_eval"))
    cat = patch(ref_import.load("PLC/PLC1_low_mid_high_eval.py", "ref_plc1_cat"))

    # ---- G17
    g17 = {}
    for name in pe.STSIM_CASES:
        ref, est, lm = pe.stsim_case(name)
        r_, e_, m_ = torch.from_numpy(ref), torch.from_numpy(est), torch.from_numpy(lm)
        X = ev._mel_mag(r_.unsqueeze(0))[0].numpy()
        Y = ev._mel_mag(e_.unsqueeze(0))[0].numpy()
        n_frames, T_wave, T_lat = X.shape[1], ref.shape[-1], lm.size
        if T_lat:
            spt = float(T_wave) / float(T_lat)
            tok = np.clip(np.floor((np.arange(n_frames) * ev.MEL_HOP) / spt).astype(np.int64), 0, T_lat - 1)
            g17[f"{name}.frame_mask"] = lm[tok]
        else:
            g17[f"{name}.frame_mask"] = np.zeros(n_frames, bool)
        g17[f"{name}.X"], g17[f"{name}.Y"] = X, Y
        for branch, sk in (("ssim", True), ("norm", False)):
            with Branch((ev, cat), sk):
                g17[f"{name}.{branch}.with_mask"] = np.array(ev.compute_stsim_mel_with_mask(r_, e_, m_), np.float64)
                g17[f"{name}.{branch}.global"] = np.array(cat.compute_stsim_mel_global(r_, e_), np.float64)
    np.savez_compressed(OUT / "g17_plc_stsim.npz", **g17)

    # ---- G18: pass 1 of eval_model on two files
    da, dt = T.DAC(), T.DAC()
    net = ev.AllPredPLC(da.encoder, da.quantizer, dt.encoder, dt.decoder, c_lat=1024)
    net.load_state_dict(pi.plc_state(), strict=True)
    net.eval()
    files = {n: pe.eval_file(n) for n in pe.EVAL_FILES}
    peak = max(max(float(np.abs(t).max()) for _, t, _ in files.values()), 0.0) or 1.0      # compute_global_peak
    g18 = {"peak": np.array(peak, np.float64)}
    orig = ev.make_token_loss_mask
    for name, (a, t, lm) in files.items():
        aw_raw, tw_raw = torch.from_numpy(a), torch.from_numpy(t)
        asr = tsr = ev.TARGET_SR
        scale = max(float(tw_raw.abs().max().cpu()), 1e-8)
        aw_24 = ev.resample_to(aw_raw, asr, ev.TARGET_SR)[:1, :]
        tw_24_norm = ev.resample_to(tw_raw / scale, tsr, ev.TARGET_SR)[:1, :]
        L = min(aw_24.shape[-1], tw_24_norm.shape[-1])
        a_1T = ev.sanitize_wave(aw_24[..., :L]).unsqueeze(0)
        t_1T = ev.sanitize_wave(tw_24_norm[..., :L]).unsqueeze(0)
        mask = torch.from_numpy(lm).unsqueeze(0)
        ev.make_token_loss_mask = lambda batch_size, T_lat, packet_tok, p_loss, device: mask.to(device)
        try:
            out = net.forward_step(a_1T, t_1T)
        finally:
            ev.make_token_loss_mask = orig
        y_hat_norm = out["y_hat"].detach().cpu()[0, 0, :]
        latent_mask = out["latent_mask"].detach().cpu()[0, 0, :].bool()
        assert torch.equal(latent_mask, mask[0])
        ref_24 = ev.resample_to(tw_raw, tsr, ev.TARGET_SR)[0].cpu()
        est_24 = y_hat_norm * scale
        ref_c, est_c = ev.crop_match(ref_24.unsqueeze(0), est_24.unsqueeze(0))
        ref_a, est_a, best_shift = ev.align_by_xcorr(ref_c, est_c, ev.MAX_ALIGN_SHIFT)
        ref_a, est_a = ev.crop_match(ref_a, est_a)
        row = {"len_samples": float(ref_a.numel()), "psnr_global_db": ev.psnr_global_peak_db(ref_a, est_a, peak)}
        ref_vec, est_vec = ref_a.reshape(-1), est_a.reshape(-1)
        T_wave, T_lat = ref_vec.numel(), latent_mask.numel()
        spt = float(T_wave) / float(T_lat)
        token_idx = torch.clamp(torch.floor(torch.arange(T_wave, dtype=torch.float32) / spt).long(), 0, T_lat - 1)
        sm = latent_mask[token_idx]
        row["mae_masked"], row["mae_unmasked"] = ev.mae_subset(ref_vec, est_vec, sm), ev.mae_subset(ref_vec, est_vec, ~sm)
        row["snr_masked_db"], row["snr_unmasked_db"] = ev.snr_subset_db(ref_vec, est_vec, sm), ev.snr_subset_db(ref_vec, est_vec, ~sm)
        row["psnr_masked_db"] = ev.psnr_subset_db(ref_vec, est_vec, sm, peak)
        row["psnr_unmasked_db"] = ev.psnr_subset_db(ref_vec, est_vec, ~sm, peak)
        for branch, sk in (("ssim", True), ("norm", False)):
            with Branch((ev, cat), sk):
                g, m, u = ev.compute_stsim_mel_with_mask(ref_a, est_a, latent_mask, sr=ev.EVAL_SR)
                row.update(stsim_global=g, stsim_masked=m, stsim_unmasked=u)
                g18[f"{name}.{branch}.row"] = np.array([row[k] for k in ROW], np.float64)
        g18[f"{name}.best_shift"] = np.array(best_shift, np.int64)
        g18[f"{name}.mae_global"] = np.array(cat.mae_global(ref_a, est_a), np.float64)
        g18[f"{name}.mask"] = lm
        print(name, "shift", best_shift, dict(zip(ROW, g18[f"{name}.ssim.row"].round(5))))
    np.savez_compressed(OUT / "g18_plc_eval_rows.npz", **g18)
    for f in ("g17_plc_stsim.npz", "g18_plc_eval_rows.npz"):
        print(f, (OUT / f).stat().st_size)


if __name__ == "__main__":
    main()
