"""What the FEC tests share (tests/test_fec_cpu.py, tests/test_gpu_fec.py): the six shapes, seeded items, a seeded lossy channel
over data and parity packets, the numpy rule run end to end, and the classification of what happened to each parity group.

The expected values all come from packets.py's numpy definition (fec_rows / frame_fec / gather_fec / fec_recover) and from the
existing frame / thin / gather / unpack_bodies; nothing here looks at what a kernel returns."""
import numpy as np

from multimodal_vqvae_compression_audio_tactile_amd import packets
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, StreamInfo

# (K, nb, T, packet_tok, g, m)
SHAPES = [(512, 8, 37, 2, 4, 3),        # a 54-bit prefix: the book boundary falls inside a byte
          (1024, 32, 37, 2, 8, 4),      # the audio shape
          (37, 9, 5, 1, 2, 9),          # K not a power of two, m = nb, a tail group of one
          (128, 10, 16, 16, 1, 2),      # g = 1
          (512, 8, 75, 2, 8, 8),
          (1024, 9, 21, 4, 4, 2)]       # a tail packet of one token inside a group
OUTCOMES = ("recovered-lost", "recovered-thinned", "two-deficient", "parity-lost")


def seq_of(pkt):
    return int.from_bytes(bytes(pkt)[3:7], "little")


def item(shape, seed):
    """One seeded item -> dict(info, fec, idx, nb_sent, bodies, sent, rows, par)."""
    K, nb, T, ptok, g, m = shape
    info, fec = StreamInfo(K, nb, T, ptok), Fec(g, m)
    r = np.random.default_rng(1000 * seed + K + nb + T)
    idx = r.integers(0, K, size=(nb, T))
    nb_sent = r.integers(1, nb + 1, size=info.P)
    bodies = packets.pack_bodies(idx, info)
    rows = packets.fec_rows(bodies, nb_sent, info, fec)
    return dict(info=info, fec=fec, idx=idx, nb_sent=nb_sent, bodies=bodies, sent=packets.frame(bodies, info, nb_sent=nb_sent),
                rows=rows, par=packets.frame_fec(rows, info, fec))


def channel(sent, par, info, seed, drop=0.20, thin=0.15, par_loss=0.15):
    """A seeded channel: each data packet is dropped (20 %) or thinned by a relay (15 %, to 1 .. nb_sent - 1 books), what is left
    is reordered and two packets are duplicated (one of them as a poorer copy); each parity packet is lost with 15 %, the rest
    reversed with a duplicate -> (data packets that arrive, parity packets that arrive)."""
    r = np.random.default_rng(seed)
    out = []
    for p in sent:
        u = r.uniform()
        if u < drop:
            continue
        if u < drop + thin and p[8] > 1:
            p = packets.thin(p, int(r.integers(1, p[8])), info)
        out.append(p)
    out = [out[i] for i in r.permutation(len(out))]
    if out:
        out.append(out[0])
        if out[-1][8] > 1:
            out.append(packets.thin(out[-1], 1, info))
    pout = [p for p in par if r.uniform() >= par_loss][::-1]
    if pout:
        pout.append(pout[0])
    return out, pout


def rule(recv, recv_par, info, fec):
    """The numpy receiver: gather, gather_fec, fec_recover -> dict(b0, r0 (as gathered), rows, got, b1, r1, rec (after recovery))."""
    b0, r0 = packets.gather(recv, info)
    rows, got = packets.gather_fec(recv_par, info, fec)
    b1, r1, rec = packets.fec_recover(b0, r0, rows, got, info, fec)
    return dict(b0=b0, r0=r0, rows=rows, got=got, b1=b1, r1=r1, rec=rec)


def outcomes(nb_sent, r0, got, info, fec):
    """What happened to each parity group with something deficient -> the set of OUTCOMES names that occurred."""
    g, m, G, _ = fec.resolve(info)
    seen = set()
    for j in range(G):
        grp = range(j * g, min(info.P, (j + 1) * g))
        bad = [p for p in grp if int(r0[p]) < min(m, int(nb_sent[p]))]
        if not bad:
            continue
        if not got[j]:
            seen.add("parity-lost")
        elif len(bad) >= 2:
            seen.add("two-deficient")
        else:
            seen.add("recovered-lost" if r0[bad[0]] == 0 else "recovered-thinned")
    return seen


def repaired(sent, recv, rec, nb_sent, info, fec):
    """``recv`` with every packet the rule recovers replaced by packets.thin(sent_packet, c_q): the list plain decompress_packets
    must decode to the same output."""
    out = [p for p in recv if not rec[seq_of(p)]]
    for q in np.flatnonzero(rec):
        out.append(packets.thin(sent[q], min(int(fec.books), int(nb_sent[q])), info))
    return out
