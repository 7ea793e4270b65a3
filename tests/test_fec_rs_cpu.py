"""CPU: Reed-Solomon forward error correction as packets.py defines it (Fec.parity = r, fec_rows / frame_fec / gather_fec /
fec_recover), on the six shapes of tests/fec_rs_channel.py.  Every comparison is an equality.

  * the field GF(2^8) / 0x11d and the exhaustive check that every square submatrix of A (4 x 16) is nonsingular: the limits
    parity <= 4 and group <= 16, and elimination without pivoting, rest on it;
  * parity = 1 IS today's code: the same arrays, packets and recoveries; the ``MF`` packets of a parity = r stream are the parity
    packets of the XOR stream;
  * the yardstick that does not know the field: every packet the rule marks recovered is the body of thin(sent_packet, c_q);
    every other row and count is untouched;
  * every erasure pattern of one group: |D| <= |arrived| recovers all of D (also without parity 0), |D| > |arrived| changes nothing;
  * THE CONDITION the GPU kernel tests rely on: their seeded inputs contain each of the eight outcomes;
  * gather_fec's refusals, duplicates, ``late``; fec_bits against the framed lengths."""
import dataclasses
import itertools

import numpy as np
import pytest

import fec_channel as fc
import fec_rs_channel as rc
from multimodal_vqvae_compression_audio_tactile_amd import packets
from multimodal_vqvae_compression_audio_tactile_amd.packets import Fec, StreamInfo


# ------------------------------------------------------------------------------------------------------------------- the field
def _mul_slow(a, b):
    """The product by shift-and-xor, independent of the tables."""
    acc = 0
    for s in range(8):
        if b >> s & 1:
            acc ^= a
        a = (a << 1) ^ (0x11d if a & 0x80 else 0)
    return acc


def test_the_field():
    assert packets.GF_EXP.dtype == np.uint8 and packets.GF_EXP.shape == (512,) and packets.GF_LOG.shape == (256,)
    assert packets.GF_EXP[0] == 1 and packets.GF_EXP[1] == 2 and packets.GF_EXP[8] == 0x1d
    assert sorted(int(v) for v in packets.GF_EXP[:255]) == list(range(1, 256))          # 2 generates the whole group
    for a in range(1, 256):
        assert int(packets.gf_mul(a, packets.gf_inv(a))) == 1
    with pytest.raises(ZeroDivisionError):
        packets.gf_inv(0)
    rng = np.random.default_rng(11)
    a, b, c = (rng.integers(0, 256, size=4096).astype(np.uint8) for _ in range(3))
    a[:8], b[8:16] = 0, 0
    assert np.array_equal(packets.gf_mul(a, b ^ c), packets.gf_mul(a, b) ^ packets.gf_mul(a, c))      # distributivity
    assert np.array_equal(packets.gf_mul(a, b), packets.gf_mul(b, a))
    assert np.array_equal(packets.gf_mul(a, b), np.array([_mul_slow(int(x), int(y)) for x, y in zip(a, b)], np.uint8))
    for i in range(packets.FEC_MAX_PARITY):
        for u in range(packets.FEC_MAX_GROUP):
            want = 1
            for _ in range(i * u):
                want = _mul_slow(want, 2)
            assert packets.fec_coef(i, u) == want
    assert all(packets.fec_coef(0, u) == 1 for u in range(16))            # parity 0 is the XOR row


def _det(mat):
    """The determinant of a small matrix over GF(2^8), by elimination WITH pivoting (independent of gf_solve_matrix)."""
    mat, det = [list(row) for row in mat], 1
    for k in range(len(mat)):
        piv = next((e for e in range(k, len(mat)) if mat[e][k]), None)
        if piv is None:
            return 0
        mat[k], mat[piv] = mat[piv], mat[k]
        det = _mul_slow(det, mat[k][k])
        inv = packets.gf_inv(mat[k][k])
        for e in range(k + 1, len(mat)):
            f = _mul_slow(mat[e][k], inv)
            mat[e] = [v ^ _mul_slow(f, w) for v, w in zip(mat[e], mat[k])]
    return det


def test_every_square_submatrix_of_the_code_is_nonsingular():
    """4844 submatrices, none singular: any d erasures are solvable from any d arrived parities, and the leading minors of each
    system (submatrices themselves) are nonzero, so Gauss-Jordan needs no pivoting."""
    n = singular = 0
    for d in range(1, packets.FEC_MAX_PARITY + 1):
        for idx in itertools.combinations(range(packets.FEC_MAX_PARITY), d):
            for cols in itertools.combinations(range(packets.FEC_MAX_GROUP), d):
                n += 1
                singular += _det([[packets.fec_coef(i, q) for q in cols] for i in idx]) == 0
    assert (n, singular) == (4844, 0)
    rng = np.random.default_rng(5)                                        # gf_solve_matrix returns the inverse
    for _ in range(50):
        d = int(rng.integers(1, 5))
        idx, cols = sorted(rng.choice(4, d, replace=False)), sorted(rng.choice(16, d, replace=False))
        inv = packets.gf_solve_matrix(idx, cols)
        for a in range(d):
            for b in range(d):
                acc = 0
                for k in range(d):
                    acc ^= _mul_slow(packets.fec_coef(idx[a], cols[k]), int(inv[k, b]))
                assert acc == int(a == b)


# ------------------------------------------------------------------------------------------------------------ the value itself
def test_the_fec_value():
    assert Fec(4, 3) == Fec(4, 3, 1) and Fec(4, 3).parity == 1 and Fec(4, 3) != Fec(4, 3, 2)
    assert repr(Fec(4, 3, 1)) == "Fec(group=4, books=3)" and repr(Fec(8, 3, 2)) == "Fec(group=8, books=3, parity=2)"
    assert packets.FEC_MAX_PARITY == 4 and Fec(8, 3, 4).r == 4
    info = StreamInfo(512, 8, 37, 2)
    assert Fec(4, 3, 2).resolve(info) == Fec(4, 3).resolve(info)
    assert Fec(4, 3).rows_shape(info) == (5, 4 + 7) and Fec(4, 3, 3).rows_shape(info) == (5, 3, 4 + 7)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError, match="parity"):
            Fec(4, 3, bad).resolve(info)
        with pytest.raises(ValueError, match="parity"):
            packets.fec_rows(np.zeros((19, 18), np.uint8), None, info, Fec(4, 3, bad))
    for bad in (True, 2.0, "2"):
        with pytest.raises(ValueError, match="parity"):
            Fec(4, 3, bad)
    with pytest.raises(dataclasses.FrozenInstanceError):
        Fec(4, 3, 2).parity = 3


# ----------------------------------------------------------------------------------------------------- parity = 1 is today's
@pytest.mark.parametrize("shape", fc.SHAPES)
def test_parity_one_is_the_xor_code(shape):
    K, nb, T, ptok, g, m = shape
    for seed in range(3):
        it = fc.item(shape, seed)
        info, f0, f1 = it["info"], it["fec"], Fec(g, m, 1)
        rows = packets.fec_rows(it["bodies"], it["nb_sent"], info, f1)
        assert rows.shape == it["rows"].shape and np.array_equal(rows, it["rows"])
        assert packets.frame_fec(rows, info, f1) == it["par"] and packets.frame_fec(rows, info, f1, seq_base=7) == \
            packets.frame_fec(it["rows"], info, f0, seq_base=7)
        assert packets.fec_bits(info, f1, it["nb_sent"]) == packets.fec_bits(info, f0, it["nb_sent"])
        recv, recv_par = fc.channel(it["sent"], it["par"], info, 77 * seed + 5)
        o = fc.rule(recv, recv_par, info, f0)
        r1, g1 = packets.gather_fec(recv_par, info, f1)
        assert r1.shape == o["rows"].shape and np.array_equal(r1, o["rows"]) and np.array_equal(g1, o["got"]) and set(g1) <= {0, 1}
        out = packets.fec_recover(o["b0"], o["r0"], r1, g1, info, f1)
        for a, b in zip(out, (o["b1"], o["r1"], o["rec"])):
            assert np.array_equal(a, b)
        # and both are the XOR code restated without the field (tests/fec_rs_channel.py)
        assert np.array_equal(rows, rc.xor_rows(it["bodies"], it["nb_sent"], info, g, m))
        for a, b in zip(out, rc.xor_recover(o["b0"], o["r0"], r1, g1, info, g, m)):
            assert np.array_equal(a, b)
        for r in (2, 4):                                                  # the MF packets of a parity = r stream: an XOR-only receiver's
            fr = Fec(g, m, r)
            par = packets.frame_fec(packets.fec_rows(it["bodies"], it["nb_sent"], info, fr), info, fr)
            assert len(par) == r * len(it["par"]) and [p for p in par if p[:2] == b"MF"] == it["par"]
            assert par[0::r] == it["par"] and all(p[:2] == b"MR" and p[9] == k % r for k, p in enumerate(par) if k % r)
            with pytest.raises(ValueError, match="magic"):                # and refuses the rest by their magic
                packets.gather_fec(par, info, f1)
            with pytest.raises(ValueError, match="magic"):
                packets.gather(par[:1], info)
            with pytest.raises(ValueError, match="magic"):
                packets.gather(par[1:2], info)


# ------------------------------------------------------------------------------------------- the yardstick: thin(sent, c_q)
def _thinned_row(sent_packet, c, info):
    """Row and count that gathering thin(sent_packet, c) alone gives: the definition of a recovered packet."""
    b, r = packets.gather([packets.thin(sent_packet, c, info)], info)
    q = rc.seq_of(sent_packet)
    return b[q], int(r[q])


def _check_against_thin(it, o):
    """Every packet marked recovered equals thin(sent, c_q); every other row and count is as it arrived."""
    info, fec = it["info"], it["fec"]
    m = int(fec.books)
    for p in range(info.P):
        if o["rec"][p]:
            c = min(m, int(it["nb_sent"][p]))
            row, cnt = _thinned_row(it["sent"][p], c, info)
            assert o["r0"][p] < c == cnt == o["r1"][p] and np.array_equal(o["b1"][p], row), p
        else:
            assert o["r1"][p] == o["r0"][p] and np.array_equal(o["b1"][p], o["b0"][p]), p


@pytest.mark.parametrize("shape", rc.SHAPES)
def test_the_rule_on_seeded_channels(shape):
    for seed in range(8):
        it = rc.item(shape, seed)
        info, fec = it["info"], it["fec"]
        g, m, G, W = fec.resolve(info)
        assert it["rows"].shape == (G, fec.r, g + W) and len(it["par"]) == G * fec.r
        recv, recv_par = rc.channel(it["sent"], it["par"], info, 77 * seed + 5)
        o = rc.rule(recv, recv_par, info, fec)
        assert o["rows"].shape == it["rows"].shape and o["got"].shape == (G,) and int(o["got"].max()) < 1 << fec.r
        _check_against_thin(it, o)
        for j in range(G):                                                # the decision, restated
            grp = list(range(j * g, min(info.P, (j + 1) * g)))
            bad = [p for p in grp if int(o["r0"][p]) < min(m, int(it["nb_sent"][p]))]
            arr = rc.arrived(o["got"][j], fec)
            assert list(np.flatnonzero(o["rec"][grp])) == ([grp.index(p) for p in bad] if arr and 1 <= len(bad) <= len(arr) else [])
        idx, nb_valid = packets.unpack_bodies(o["b1"], o["r1"], info)
        for t in range(info.T):                                           # every book that counts is the index sent
            assert np.array_equal(idx[:nb_valid[t], t], it["idx"][:nb_valid[t], t]), (seed, t)


def test_every_erasure_pattern_of_one_group():
    """One group of 4 packets and 3 parities: each data packet arrives, is lost, or is thinned to one book; each subset of the
    parity arrives (648 patterns)."""
    shape = (512, 8, 8, 2, 4, 3, 3)
    it = rc.item(shape, 1)
    info, fec = it["info"], it["fec"]
    assert info.P == 4
    n_fixed = n_left = 0
    for states in itertools.product((0, 1, 2), repeat=4):
        recv = []
        for p, s in enumerate(states):
            if s == 1 or (s == 2 and it["sent"][p][8] == 1):
                recv.append(it["sent"][p])
            elif s == 2:
                recv.append(packets.thin(it["sent"][p], 1, info))
        b0, r0 = packets.gather(recv, info)
        bad = [p for p in range(4) if int(r0[p]) < min(3, int(it["nb_sent"][p]))]
        for mask in range(8):
            par = [it["par"][i] for i in range(3) if mask >> i & 1]
            rows, got = packets.gather_fec(par, info, fec)
            assert got[0] == mask
            b1, r1, rec = packets.fec_recover(b0, r0, rows, got, info, fec)
            o = dict(b0=b0, r0=r0, b1=b1, r1=r1, rec=rec)
            _check_against_thin(it, o)
            if 1 <= len(bad) <= bin(mask).count("1"):
                assert list(np.flatnonzero(rec)) == bad
                n_fixed += 1
            else:
                assert not rec.any() and np.array_equal(b1, b0) and np.array_equal(r1, r0)
                n_left += 1
    assert n_fixed > 100 and n_left > 100


def test_a_corrupt_count_byte_stays_inside_the_row():
    it = rc.item(rc.SHAPES[0], 2)
    info, fec = it["info"], it["fec"]
    rows = it["rows"].copy()
    rows[0, :, 0] = 255                                                   # clamped to min(255, m, nb) = m
    b0, r0 = packets.gather(it["sent"][1:], info)
    got = np.full(rows.shape[0], 3, np.uint8)
    b1, r1, rec = packets.fec_recover(b0, r0, rows, got, info, fec)
    assert rec[0] == 1 and r1[0] == 3


# --------------------------------------------------------------------------------- the condition the GPU kernel tests rely on
def test_the_kernel_inputs_see_every_outcome():
    seen = set()
    for shape in rc.SHAPES:
        c = rc.batch(shape, 3)
        for b in range(3):
            seen |= rc.outcomes(c["nb_sent"][b], c["r0"][b], c["got"][b], c["info"], c["fec"])
    assert seen == set(rc.OUTCOMES), set(rc.OUTCOMES) - seen


# ----------------------------------------------------------------------------------------------- framing, refusals, lengths
@pytest.mark.parametrize("shape", rc.SHAPES)
def test_frame_gather_round_trip_and_length(shape):
    it = rc.item(shape, 3)
    info, fec = it["info"], it["fec"]
    g, m, G, W = fec.resolve(info)
    r = fec.r
    for k, pkt in enumerate(it["par"]):                                   # group-major: all indices of group 0, then group 1, ...
        j, i = divmod(k, r)
        grp = range(j * g, min(info.P, (j + 1) * g))
        counts = [min(m, int(it["nb_sent"][p])) for p in grp]
        n = max(packets.body_bytes(info.ntok(p), c, info.K) for p, c in zip(grp, counts))
        head = packets.HEADER_BYTES + (1 if i else 0)
        assert pkt[:2] == (b"MR" if i else b"MF") and pkt[2] == packets.VERSION and rc.seq_of(pkt) == j
        assert pkt[7] == len(grp) and pkt[8] == max(counts) and (i == 0 or pkt[9] == i)
        assert list(pkt[head:head + len(grp)]) == counts and len(pkt) == head + len(grp) + n
        assert pkt[head + len(grp):] == it["rows"][j, i, g:g + n].tobytes() and not it["rows"][j, i, g + n:].any()
    assert packets.fec_bits(info, fec, it["nb_sent"]) == 8 * sum(len(p) for p in it["par"])
    assert packets.fec_bits(info, fec, it["nb_sent"], headers=False) == \
        8 * sum(len(p) - packets.HEADER_BYTES - p[7] - (p[:2] == b"MR") for p in it["par"])
    assert packets.fec_kbps(info, fec, it["nb_sent"]) == packets.fec_bits(info, fec, it["nb_sent"]) * 75.0 / (1000.0 * info.T)
    full = packets.frame_fec(packets.fec_rows(it["bodies"], None, info, fec), info, fec)
    assert packets.fec_bits(info, fec) == 8 * sum(len(p) for p in full)
    rows, got = packets.gather_fec(it["par"][::-1] + it["par"][:3], info, fec)          # reordered, duplicates: harmless
    assert np.array_equal(rows, it["rows"]) and (got == (1 << r) - 1).all()
    rows, got = packets.gather_fec(it["par"][1::r], info, fec)                          # index 1 of every group alone
    assert (got == 2).all() and np.array_equal(rows[:, 1], it["rows"][:, 1]) and not rows[:, 0].any()
    shifted = packets.frame_fec(it["rows"], info, fec, seq_base=40)                     # a chunk of a longer stream
    assert [rc.seq_of(p) for p in shifted] == [40 + k // r for k in range(G * r)]
    rows, got = packets.gather_fec(shifted, info, fec, seq_base=40)
    assert np.array_equal(rows, it["rows"])
    late = []
    rows, got = packets.gather_fec(shifted + it["par"][:2], info, fec, seq_base=40, late=late)
    assert late == it["par"][:2] and np.array_equal(rows, it["rows"])
    with pytest.raises(ValueError, match="seq_base"):
        packets.gather_fec(it["par"][:2], info, fec, seq_base=40)


def test_gather_fec_refusals():
    it = rc.item(rc.SHAPES[1], 4)                                         # r = 3
    info, fec = it["info"], it["fec"]
    par = it["par"]
    mr = bytearray(par[1])
    assert mr[:2] == b"MR" and mr[9] == 1
    for bad_index in (0, 3, 200):
        pkt = bytes(mr[:9]) + bytes([bad_index]) + bytes(mr[10:])
        with pytest.raises(ValueError, match="index"):
            packets.gather_fec([pkt], info, fec)
    with pytest.raises(ValueError, match="index"):
        packets.gather_fec([bytes(mr[:9])], info, fec)                    # no index byte at all
    with pytest.raises(ValueError, match="magic"):
        packets.gather_fec([par[1]], info, Fec(8, 4))                     # MR at parity == 1: today's bad magic
    with pytest.raises(ValueError, match="magic"):
        packets.gather_fec([it["sent"][0]], info, fec)
    with pytest.raises(ValueError, match="magic"):
        packets.gather_fec([b"MQ" + par[0][2:]], info, fec)
    with pytest.raises(ValueError, match="version"):
        packets.gather_fec([par[1][:2] + b"\x02" + par[1][3:]], info, fec)
    with pytest.raises(ValueError, match="bytes"):
        packets.gather_fec([par[1][:-1]], info, fec)
    with pytest.raises(ValueError, match="bytes"):
        packets.gather_fec([par[1] + b"\x00"], info, fec)
    with pytest.raises(ValueError, match="seq"):
        packets.gather_fec([par[1][:3] + (99).to_bytes(4, "little") + par[1][7:]], info, fec)
    with pytest.raises(ValueError, match="covers"):
        packets.gather_fec([par[1][:7] + bytes([par[1][7] - 1]) + par[1][8:]], info, fec)
    # two parity packets of one group whose count bytes disagree (each well-formed on its own)
    other = rc.item(rc.SHAPES[1], 5)
    assert other["par"][1][10:18] != par[1][10:18]
    with pytest.raises(ValueError, match="disagree"):
        packets.gather_fec([par[0], other["par"][1]], info, fec)
    with pytest.raises(ValueError, match="disagree"):
        packets.gather_fec([other["par"][2], par[1]], info, fec)
    rows, got = packets.gather_fec([par[1], par[1], par[2]], info, fec)   # duplicates of one index agree with themselves
    assert got[0] == 6
    with pytest.raises(ValueError, match="count"):
        packets.frame_fec(np.zeros_like(it["rows"]), info, fec)
    with pytest.raises(ValueError, match="parity rows"):
        packets.frame_fec(it["rows"][:-1], info, fec)
    with pytest.raises(ValueError, match="parity rows"):
        packets.fec_recover(it["bodies"], it["nb_sent"], it["rows"][:, :2], np.zeros(it["rows"].shape[0]), info, fec)


def test_the_native_surface():
    """The two exports exist with the documented signatures; the Python surface routes by parity."""
    from multimodal_vqvae_compression_audio_tactile_amd import _lib
    assert len(_lib.EXPORTS["mvq_fec_rs_parity_u8"][1]) == 12 and len(_lib.EXPORTS["mvq_fec_rs_recover_u8"][1]) == 14
    assert len(_lib.EXPORTS["mvq_fec_parity_u8"][1]) == 11 and len(_lib.EXPORTS["mvq_fec_recover_u8"][1]) == 13
