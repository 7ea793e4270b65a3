"""CPU: the packet format (packets.py) and the lossy-channel receiver's arithmetic, restated from oracle pieces
(tests/lossy_oracle.py).

  * pack / unpack / frame / gather round trips, the pinned byte layout (book-major, LSB first), thinning, every refusal;
  * the two-pass order equals the per-chunk loop bit for bit under every loss pattern (and equals the lossless receiver when
    every book arrived);
  * the indices of books that did not arrive cannot reach the output;
  * the receiver's new arguments are refused before any launch; the new operators' fakes answer with the kernels' shapes."""
import itertools

import numpy as np
import pytest
import torch

import lossy_oracle as lo
import receiver_oracle as ro
from multimodal_vqvae_compression_audio_tactile_amd import packets, synth
from multimodal_vqvae_compression_audio_tactile_amd.packets import StreamInfo


def _np(sd):
    return {k: v.numpy() for k, v in sd.items()}


def _idx(K, nb, T, seed=0):
    r = np.random.default_rng(K * 7919 + nb * 31 + T + seed)
    idx = r.integers(0, K, size=(nb, T))
    idx[:, :1] = K - 1                                               # the largest index survives
    return idx


# ------------------------------------------------------------------------------------------------------------ 1. format
@pytest.mark.parametrize("K", [1, 2, 128, 300, 512, 1024])
@pytest.mark.parametrize("nb", [1, 3, 8, 32])
def test_format_round_trips(K, nb):
    for T, ptok in itertools.product([0, 1, 2, 17, 35, 75], [1, 2, 5, 16]):
        info = StreamInfo(K, nb, T, ptok)
        idx = _idx(K, nb, T, ptok)
        bodies = packets.pack_bodies(idx, info)
        P = -(-T // ptok)
        assert info.P == P and bodies.dtype == np.uint8 and bodies.shape == (P, packets.body_bytes(ptok, nb, K))
        back, nbv = packets.unpack_bodies(bodies, np.full(P, nb), info)
        assert back.dtype == np.int64 and np.array_equal(back, idx)
        assert nbv.dtype == np.uint8 and nbv.shape == (T,) and np.all(nbv == nb)
        # framed, through gather, back to the same array
        pk = packets.frame(bodies, info)
        assert len(pk) == P
        bits = int(np.ceil(np.log2(K))) if K > 1 else 0
        for p, one in enumerate(pk):
            ntok = min(ptok, T - p * ptok)
            assert len(one) == packets.HEADER_BYTES + (nb * ntok * bits + 7) // 8
            assert one[:3] == b"MP\x01" and int.from_bytes(one[3:7], "little") == p and one[7] == ntok and one[8] == nb
        g_bodies, g_recv = packets.gather(pk, info)
        assert np.array_equal(g_bodies, bodies) and np.array_equal(g_recv, np.full(P, nb))
        # a per-packet book count: books at or above it decode as 0 and are not counted
        recv = np.arange(P) % (nb + 1)
        part, nbv = packets.unpack_bodies(bodies, recv, info)
        tok_recv = np.repeat(recv, ptok)[:T]
        assert np.array_equal(nbv, tok_recv)
        assert np.array_equal(part, np.where(np.arange(nb)[:, None] < tok_recv[None, :], idx, 0))


def test_body_length_is_the_rate():
    assert packets.body_bytes(2, 8, 512) == 18                       # 8 books x 9 bits x 2 tokens = 144 bits
    assert packets.body_bytes(2, 1, 512) == 3 and packets.body_bytes(1, 8, 512) == 9
    assert packets.body_bytes(5, 10, 128) == 44 and packets.body_bytes(16, 3, 300) == 54
    assert packets.body_bytes(2, 8, 1) == 0 and packets.body_bytes(0, 8, 512) == 0
    info = StreamInfo(512, 8, 75)
    assert info.packet_tok == 2 and info.P == 38 and info.ntok(37) == 1 and info.ntok(0) == 2
    from multimodal_vqvae_compression_audio_tactile_amd import plc
    assert packets.PACKET_TOK == plc.PACKET_TOK


def test_bit_layout_is_book_major_lsb_first():
    idx = np.array([[1, 2, 3], [3, 0, 1]])                           # nb = 2, T = 3, K = 4 (2 bits), packets of 2 tokens
    bodies = packets.pack_bodies(idx, StreamInfo(4, 2, 3, 2))
    # packet 0, tokens 0-1: book0 = 1, 2 then book1 = 3, 0 -> bits 10 01 11 00 from the LSB -> 0b00_11_10_01
    # packet 1, token 2 alone: book0 = 3, book1 = 1 -> 0b01_11, the row zero-padded
    assert bodies.tolist() == [[0b00111001], [0b0111]]
    # an index that straddles a byte: K = 512 (9 bits), one book, tokens 0x1FF and 0x001 -> bits 0-8 set, bit 9 set
    bodies = packets.pack_bodies(np.array([[0x1FF, 0x001]]), StreamInfo(512, 1, 2, 2))
    assert bodies.tolist() == [[0xFF, 0x03, 0x00]]
    pk = packets.frame(bodies, StreamInfo(512, 1, 2, 2))
    assert pk == [b"MP\x01\x00\x00\x00\x00\x02\x01\xff\x03\x00"]


@pytest.mark.parametrize("K,nb,T,ptok", [(512, 8, 75, 2), (128, 10, 35, 5), (300, 3, 17, 16), (2, 3, 5, 2), (1, 3, 5, 2)])
def test_thin_equals_packing_the_first_books_afresh(K, nb, T, ptok):
    info = StreamInfo(K, nb, T, ptok)
    idx = _idx(K, nb, T)
    pk = packets.frame(packets.pack_bodies(idx, info), info)
    for keep in range(1, nb + 1):
        small = StreamInfo(K, keep, T, ptok)
        fresh = packets.frame(packets.pack_bodies(idx[:keep], small), small)
        thinned = [packets.thin(p, keep, info) for p in pk]
        assert thinned == fresh
        assert packets.frame(packets.pack_bodies(idx, info), info, nb_sent=keep) == fresh
        # the thinned stream decodes to the kept books, the others as 0
        bodies, recv = packets.gather(thinned, info)
        back, nbv = packets.unpack_bodies(bodies, recv, info)
        assert np.all(recv == keep) and np.all(nbv == keep)
        assert np.array_equal(back[:keep], idx[:keep]) and not back[keep:].any()
    with pytest.raises(ValueError):
        packets.thin(pk[0], 0, info)
    with pytest.raises(ValueError):
        packets.thin(packets.thin(pk[0], 1, info), 2, info)                  # books that were dropped do not come back


def test_gather_shuffled_duplicated_missing():
    info = StreamInfo(512, 8, 75, 2)
    idx = _idx(512, 8, 75)
    bodies = packets.pack_bodies(idx, info)
    pk = packets.frame(bodies, info)
    r = np.random.default_rng(3)
    missing = {4, 5, 20, 37}                                        # 37 is the one-token tail packet
    thin_to = {7: 1, 8: 3, 30: 7}
    stream = []
    for p in r.permutation(info.P):
        if p in missing:
            continue
        stream.append(packets.thin(pk[p], thin_to[p], info) if p in thin_to else pk[p])
    stream += [packets.thin(pk[10], 2, info), pk[11], packets.thin(pk[8], 1, info)]          # duplicates: poorer copies after
    stream = [packets.thin(pk[12], 4, info), packets.thin(pk[7], 1, info)] + stream            # ... and before the richer one
    got_b, got_r = packets.gather(iter(stream), info)
    want_r = np.array([0 if p in missing else thin_to.get(p, 8) for p in range(info.P)], np.uint8)
    assert got_r.dtype == np.uint8 and np.array_equal(got_r, want_r)
    back, nbv = packets.unpack_bodies(got_b, got_r, info)
    tok_r = np.repeat(want_r, 2)[:75]
    assert np.array_equal(nbv, tok_r)
    assert np.array_equal(back, np.where(np.arange(8)[:, None] < tok_r[None, :], idx, 0))
    for p in range(info.P):                                          # rows: the packed first books, zero beyond
        small = StreamInfo(512, int(want_r[p]), 75, 2)
        row = packets.pack_bodies(idx[:want_r[p]], small)[p] if want_r[p] else np.zeros(0, np.uint8)
        assert np.array_equal(got_b[p, :row.size], row) and not got_b[p, row.size:].any()
    # nothing received at all; T = 0
    b0, r0 = packets.gather([], info)
    assert b0.shape == (38, 18) and not b0.any() and not r0.any()
    e = StreamInfo(512, 8, 0, 2)
    assert packets.gather([], e)[0].shape == (0, 18) and packets.unpack_bodies(np.zeros((0, 18), np.uint8), [], e)[0].shape == (8, 0)


def test_gather_rejects_bad_packets():
    info = StreamInfo(128, 3, 5, 2)                                  # P = 3, the tail packet has 1 token
    pk = packets.frame(packets.pack_bodies(_idx(128, 3, 5), info), info)
    good = pk[0]

    def bad(b, match):
        with pytest.raises(ValueError, match=match):
            packets.gather([good, b], info)

    bad(b"XP" + good[2:], "magic")
    bad(good[:2] + b"\x02" + good[3:], "version")
    bad(good[:3] + (3).to_bytes(4, "little") + good[7:], "seq")
    bad(good[:3] + (2).to_bytes(4, "little") + good[7:], "ntok")             # packet 2 carries one token, this one says two
    bad(good[:7] + b"\x01" + good[8:], "ntok")
    bad(good[:8] + b"\x00" + good[9:], "nb_sent")
    bad(good[:8] + b"\x04" + good[9:], "nb_sent")
    bad(good[:-1], "header implies")
    bad(good + b"\x00", "header implies")
    bad(good[:8] + b"\x02" + good[9:], "header implies")                     # the count patched without truncating the body
    bad(good[:5], "shorter")
    with pytest.raises(ValueError):
        packets.pack_bodies(np.array([[0, 128]]), StreamInfo(128, 1, 2, 2))
    with pytest.raises(ValueError):
        packets.pack_bodies(np.zeros((3, 4), np.int64), info)
    with pytest.raises(ValueError):
        packets.frame(np.zeros((3, 6), np.uint8), info, nb_sent=4)
    with pytest.raises(ValueError):
        packets.gather([], StreamInfo(128, 3, 5, 0))
    # a corrupt body cannot yield an index >= K: K = 300 takes 9 bits, all-ones is 511
    k300 = StreamInfo(300, 1, 2, 2)
    back, _ = packets.unpack_bodies(np.full((1, 3), 0xFF, np.uint8), [1], k300)
    assert back.tolist() == [[299, 299]]


# ----------------------------------------------------------------------------------- 2. two-pass equals the loop under loss
def _rand_inputs(seed, B, Ta, Tlat, nb, K):
    r = np.random.default_rng(seed)
    qa = (0.5 * r.standard_normal((B, 1024, Ta))).astype(np.float32)
    idx = r.integers(0, K, size=(nb, B, Tlat))
    return qa, idx


@pytest.fixture(scope="module")
def head_sd():
    return _np(synth.proposed_head_state(17, rvq_books=3, rvq_embed=128))


@pytest.mark.parametrize("B,Ta,Tlat", [(2, 35, 35), (1, 20, 35), (1, 0, 35), (2, 75, 75), (1, 17, 17)])
def test_two_pass_equals_chunk_loop_under_loss(B, Ta, Tlat, orc, head_sd):
    """Loss changes qD alone; pass 2 reads z_run[s-1], the last token of a full chunk, which no pass-2 result replaces: the two
    dependent passes give the loop's bits under every pattern."""
    qa, idx = _rand_inputs(Ta * 100 + Tlat, B, Ta, Tlat, 3, 128)
    for name in lo.PATTERNS:
        nbv = lo.loss_pattern(name, B, Tlat, 3)
        want = lo.lossy_loop(orc, head_sd, qa, idx, nbv)
        got = lo.lossy_two_pass(orc, head_sd, qa, idx, nbv)
        assert np.array_equal(got, want), name
        if name == "none":
            assert np.array_equal(want, ro.receiver_loop(orc, head_sd, qa, idx))
        if name == "thin1":
            assert np.array_equal(want, ro.receiver_loop(orc, head_sd, qa, idx, 1))      # a thinned token is a lower-rate token
        if name == "all":                                                                # nothing but the prediction is left
            assert np.array_equal(want, lo.lossy_loop(orc, head_sd, qa, np.zeros_like(idx), nbv))


def test_loss_patterns_are_what_they_say():
    assert lo.loss_pattern("tok15", 1, 35, 3)[0].tolist() == [3] * 15 + [0] + [3] * 19
    assert lo.loss_pattern("tok16", 1, 17, 3)[0].tolist() == [3] * 16 + [0]
    assert lo.loss_pattern("tail_packet", 1, 35, 3)[0].tolist() == [3] * 34 + [0]
    assert lo.loss_pattern("tail_packet", 1, 6, 3)[0].tolist() == [3] * 4 + [0, 0]
    assert lo.loss_pattern("alternating", 2, 7, 3)[1].tolist() == [3, 3, 0, 0, 3, 3, 0]
    assert lo.loss_pattern("thin1", 1, 3, 3)[0].tolist() == [1, 1, 1]


# -------------------------------------------------------------------------------------------- 3. lost indices cannot leak
def test_lost_indices_cannot_leak(orc, head_sd):
    B, Tlat = 2, 35
    qa, idx = _rand_inputs(77, B, Tlat, Tlat, 3, 128)
    r = np.random.default_rng(78)
    nbv = r.integers(0, 4, size=(B, Tlat)).astype(np.uint8)
    nbv[:, [0, 15, 16, 34]] = 0
    want = lo.lossy_two_pass(orc, head_sd, qa, idx, nbv)
    absent = np.arange(3)[:, None, None] >= nbv[None]
    other = np.where(absent, (idx + 1 + r.integers(0, 127, size=idx.shape)) % 128, idx)
    assert (other != idx)[absent].all() and np.array_equal(other[~absent], idx[~absent])
    assert np.array_equal(lo.lossy_two_pass(orc, head_sd, qa, other, nbv), want)
    assert np.array_equal(lo.lossy_loop(orc, head_sd, qa, other, nbv), want)
    garbage = np.where(absent, 10 ** 9, idx)                          # not even a valid index
    assert np.array_equal(lo.dequant_layers(ro.books_of(head_sd), garbage, nbv), lo.dequant_layers(ro.books_of(head_sd), idx, nbv))


# ------------------------------------------------------------------------------------- 4. refusals before any launch; fakes
def test_lossy_arguments_are_refused_before_any_launch():
    """On a CPU-resident model nothing can have been launched: the checks come first."""
    from multimodal_vqvae_compression_audio_tactile_amd import MvqError, build_proposed
    net = build_proposed(None, rvq_books=2, rvq_embed=128, device="cpu")
    idx = torch.zeros(2, 2, 20, dtype=torch.int64)
    codes = torch.zeros(2, 32, 20, dtype=torch.int64)
    full = torch.full((2, 20), 2, dtype=torch.uint8)
    with pytest.raises(MvqError, match="needs plc"):
        net.decode_latents(codes, idx, nb_valid=full, conceal="plc")
    with pytest.raises(MvqError, match="needs plc"):
        net.decode(codes, idx, nb_valid=full, conceal="plc")
    with pytest.raises(MvqError, match="conceal must be"):
        net.decode_latents(codes, idx, nb_valid=full, conceal="interpolate")
    with pytest.raises(MvqError, match="conceal must be"):
        net.decode_latents(codes, idx, conceal="none")
    for wrong in (torch.zeros(2, 19, dtype=torch.uint8), torch.zeros(1, 20, dtype=torch.uint8), torch.zeros(20, dtype=torch.uint8),
                  torch.zeros(2, 1, 20, dtype=torch.bool)):
        with pytest.raises(MvqError, match="nb_valid"):
            net.decode_latents(codes, idx, nb_valid=wrong)
    with pytest.raises(MvqError, match="uint8 or bool"):
        net.decode_latents(codes, idx, nb_valid=full.float())
    with pytest.raises(MvqError, match="uint8 or bool"):
        net.decode_latents(codes, idx, nb_valid=full.numpy())
    with pytest.raises(MvqError, match="tactile_only"):
        net.decode_latents(None, idx, tactile_only=True, nb_valid=full, conceal="plc", plc=net)
    with pytest.raises(MvqError, match="audio tokens"):
        net.decode_latents(idx=idx, qa=torch.zeros(2, 1024, 0), nb_valid=full, conceal="plc", plc=net)
    with pytest.raises(MvqError, match="attention_seq"):
        big = torch.zeros(2, 1, 8193, dtype=torch.int64)
        net.decode_latents(torch.zeros(1, 32, 8193, dtype=torch.int64), big, nb_valid=torch.zeros(1, 8193, dtype=torch.uint8),
                           conceal="plc", plc=net)
    # the ops refuse host tensors too
    from multimodal_vqvae_compression_audio_tactile_amd import ops
    with pytest.raises(MvqError):
        ops.idx_pack_packets(idx, 128, 2)
    with pytest.raises(MvqError):
        ops.idx_unpack_packets(torch.zeros(2, 10, 4, dtype=torch.uint8), torch.zeros(2, 10, dtype=torch.uint8), 128, 2, 20, 2)
    with pytest.raises(MvqError):
        ops.rvq_dequant_layers(idx, torch.zeros(2, 128, 96), full)


def test_lossy_entry_points_exist():
    from multimodal_vqvae_compression_audio_tactile_amd import ProposedEval, _lib, ops
    for n in ("compress_packets", "decompress_packets"):
        assert callable(getattr(ProposedEval, n, None)), n
    for n in ("idx_pack_packets", "idx_unpack_packets", "rvq_dequant_layers"):
        assert callable(getattr(ops, n, None)), n
    lib = _lib.lib()
    for n in ("mvq_idx_pack_packets_u8", "mvq_idx_unpack_packets", "mvq_rvq_dequant_layers_f32"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert lib.mvq_abi_version() == 3
    # refused before any device access (no GPU here): more than 24 bits, no tokens per packet, a negative size
    assert lib.mvq_idx_pack_packets_u8(None, None, 1, 1, 4, 2 ** 24 + 1, 2, 4, 4, None) == -1
    assert b"bad shape" in lib.mvq_last_error()
    assert lib.mvq_idx_pack_packets_u8(None, None, 1, 1, 4, 512, 0, 4, 4, None) == -1
    assert lib.mvq_idx_unpack_packets(None, None, None, None, 1, 1, 4, 2 ** 25, 2, None) == -1
    assert lib.mvq_idx_unpack_packets(None, None, None, None, 1, 1, 4, 512, 0, None) == -1
    assert lib.mvq_idx_unpack_packets(None, None, None, None, -1, 1, 4, 512, 2, None) == -1
    assert b"bad shape" in lib.mvq_last_error()
    assert lib.mvq_rvq_dequant_layers_f32(None, None, None, None, 1, 95, 4, 1, 128, 0, 0, None) == -1
    # zero-sized problems: 0 without a launch
    assert lib.mvq_idx_pack_packets_u8(None, None, 0, 8, 75, 512, 2, 0, 75, None) == 0
    assert lib.mvq_idx_pack_packets_u8(None, None, 3, 8, 0, 512, 2, 0, 0, None) == 0
    assert lib.mvq_idx_pack_packets_u8(None, None, 3, 8, 75, 1, 2, 225, 75, None) == 0            # K = 1: 0-bit bodies
    assert lib.mvq_idx_unpack_packets(None, None, None, None, 0, 8, 75, 512, 2, None) == 0
    assert lib.mvq_idx_unpack_packets(None, None, None, None, 3, 8, 0, 512, 2, None) == 0


def test_lossy_torch_ops_fakes():
    import multimodal_vqvae_compression_audio_tactile_amd.torch_ops as T
    o = torch.ops.mi355x_vqvae
    for n in ("rvq_dequant_layers", "idx_pack_packets", "idx_unpack_packets"):
        assert n in T.REGISTERED and hasattr(o, n), n
    m = lambda *s, dtype=torch.float32: torch.empty(*s, device="meta", dtype=dtype)
    assert o.rvq_dequant_layers(m(3, 6, 75, dtype=torch.int64), m(8, 512, 96), m(6, 75, dtype=torch.uint8), 3).shape == (6, 96, 75)
    b = o.idx_pack_packets(m(8, 6, 75, dtype=torch.int64), 512, 2, 0)
    assert b.shape == (6, 38, 18) and b.dtype == torch.uint8
    b = o.idx_pack_packets(m(6, 32, 75, dtype=torch.int64), 1024, 5, 1)
    assert b.shape == (6, 15, 200)
    idx, nbv = o.idx_unpack_packets(m(6, 38, 18, dtype=torch.uint8), m(6, 38, dtype=torch.uint8), 512, 8, 75, 2)
    assert idx.shape == (8, 6, 75) and idx.dtype == torch.int64 and nbv.shape == (6, 75) and nbv.dtype == torch.uint8
