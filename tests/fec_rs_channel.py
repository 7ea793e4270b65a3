"""What the Reed-Solomon FEC tests share (tests/test_fec_rs_cpu.py, tests/test_gpu_fec_rs.py): the six shapes, seeded items, the
seeded channel of tests/fec_channel.py (every data packet dropped or thinned, every parity packet of every index lost
independently), the numpy rule run end to end, and the classification of what happened to each parity group.

The expected values all come from packets.py's numpy definition (fec_rows / frame_fec / gather_fec / fec_recover with
Fec.parity) and from the existing frame / thin / gather / unpack_bodies; nothing here looks at what a kernel returns."""
import numpy as np

import fec_channel as fc
from multimodal_vqvae_compression_audio_tactile_amd import packets
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, StreamInfo

# (K, nb, T, packet_tok, g, m, r)
SHAPES = [(512, 8, 37, 2, 4, 3, 2),       # a book boundary inside a byte, a tail group of 3
          (1024, 32, 37, 2, 8, 4, 3),     # the audio shape; a tail group of 3 is no larger than r
          (37, 9, 5, 1, 2, 9, 2),         # r == g, a tail group of one
          (128, 10, 16, 16, 1, 2, 2),     # g == 1
          (512, 8, 75, 2, 8, 8, 4),       # the item shape at the largest r
          (512, 8, 40, 1, 16, 2, 4)]      # u up to 15; groups of 16, 16, 8
OUTCOMES = ("one-recovered", "several-recovered", "recovered-without-parity-0", "lost-and-thinned-together", "deficient-equals-arrived",
            "deficient-below-arrived", "too-many-deficient", "all-parity-lost")
PAR_LOSS = 0.30                           # every parity packet, whatever its index, is lost with 30 %

seq_of, rule, repaired = fc.seq_of, fc.rule, fc.repaired


def xor_rows(bodies, nb_sent, info, g, m):
    """The XOR parity rows uint8[G, g + W] restated without the field: what fec_rows returned before ``parity`` existed."""
    W = packets.body_bytes(info.packet_tok, m, info.K)
    rows = np.zeros(((info.P + g - 1) // g, g + W), np.uint8)
    for p in range(info.P):
        j, c = p // g, min(m, int(nb_sent[p]))
        body = np.frombuffer(packets.thin(packets.frame(bodies, info, nb_sent=nb_sent)[p], c, info)[packets.HEADER_BYTES:], np.uint8)
        rows[j, p - j * g] = c
        rows[j, g:g + len(body)] ^= body
    return rows


def xor_recover(bodies, nb_recv, rows, got, info, g, m):
    """The one-erasure rule restated without the field: what fec_recover did before ``parity`` existed."""
    bodies, nb_recv, rec = np.array(bodies, np.uint8), np.array(nb_recv, np.uint8), np.zeros(info.P, np.uint8)
    W = rows.shape[1] - g
    for j in range(rows.shape[0]):
        grp = range(j * g, min(info.P, (j + 1) * g))
        c = {p: min(int(rows[j, p - j * g]), m, info.nb) for p in grp}
        bad = [p for p in grp if int(nb_recv[p]) < c[p]]
        if not got[j] or len(bad) != 1:
            continue
        x = rows[j, g:].copy()
        for p in grp:
            if p != bad[0]:
                n, used = packets.body_bytes(info.ntok(p), c[p], info.K), c[p] * info.ntok(p) * packets.index_bits(info.K)
                pre = bodies[p, :n].copy()
                if n and used - 8 * (n - 1) < 8:
                    pre[-1] &= (1 << (used - 8 * (n - 1))) - 1
                x[:n] ^= pre
        n = packets.body_bytes(info.ntok(bad[0]), c[bad[0]], info.K)
        bodies[bad[0]] = 0
        bodies[bad[0], :n] = x[:n]
        nb_recv[bad[0]], rec[bad[0]] = c[bad[0]], 1
    return bodies, nb_recv, rec


def item(shape, seed):
    """One seeded item -> dict(info, fec, idx, nb_sent, bodies, sent, rows, par); ``par`` is group-major, all indices."""
    K, nb, T, ptok, g, m, r = shape
    info, fec = StreamInfo(K, nb, T, ptok), Fec(g, m, r)
    rng = np.random.default_rng(1000 * seed + K + nb + T + r)
    idx = rng.integers(0, K, size=(nb, T))
    nb_sent = rng.integers(1, nb + 1, size=info.P)
    bodies = packets.pack_bodies(idx, info)
    rows = packets.fec_rows(bodies, nb_sent, info, fec)
    return dict(info=info, fec=fec, idx=idx, nb_sent=nb_sent, bodies=bodies, sent=packets.frame(bodies, info, nb_sent=nb_sent),
                rows=rows, par=packets.frame_fec(rows, info, fec))


def channel(sent, par, info, seed, par_loss=PAR_LOSS):
    """fec_channel.channel: data packets dropped (20 %) or thinned (15 %), reordered, duplicated; each parity packet lost
    independently, the rest reversed with a duplicate."""
    return fc.channel(sent, par, info, seed, par_loss=par_loss)


def batch(shape, B):
    """B seeded items over the seeded channel, the numpy rule's arrays stacked -> dict of uint8 arrays [B, ...]: the inputs of the
    GPU kernel tests."""
    items = [item(shape, b) for b in range(B)]
    info, fec = items[0]["info"], items[0]["fec"]
    outs = []
    for b, it in enumerate(items):
        recv, recv_par = channel(it["sent"], it["par"], info, 77 * b + 5)
        outs.append(rule(recv, recv_par, info, fec))
    st = lambda xs: np.stack(xs).astype(np.uint8)
    return dict(info=info, fec=fec, items=items, bodies=st([it["bodies"] for it in items]), nb_sent=st([it["nb_sent"] for it in items]),
                rows_sent=st([it["rows"] for it in items]), **{k: st([o[k] for o in outs]) for k in outs[0]})


def arrived(got_j, fec):
    """The parity indices of one group that arrived, ascending."""
    return [i for i in range(fec.r) if int(got_j) >> i & 1] if fec.r > 1 else ([0] if got_j else [])


def outcomes(nb_sent, r0, got, info, fec):
    """What happened to each parity group with something deficient -> the set of OUTCOMES names that occurred."""
    g, m, G, _ = fec.resolve(info)
    seen = set()
    for j in range(G):
        grp = range(j * g, min(info.P, (j + 1) * g))
        bad = [p for p in grp if int(r0[p]) < min(m, int(nb_sent[p]))]
        if not bad:
            continue
        arr = arrived(got[j], fec)
        if not arr:
            seen.add("all-parity-lost")
        elif len(bad) > len(arr):
            seen.add("too-many-deficient")
        else:
            seen.add("one-recovered" if len(bad) == 1 else "several-recovered")
            seen.add("deficient-equals-arrived" if len(bad) == len(arr) else "deficient-below-arrived")
            if arr[0] != 0:
                seen.add("recovered-without-parity-0")
            if any(r0[p] == 0 for p in bad) and any(r0[p] != 0 for p in bad):
                seen.add("lost-and-thinned-together")
    return seen
