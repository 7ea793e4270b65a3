"""Packet format of the tactile stream over a lossy channel (host side, numpy), next to bitstream.py's monolithic v1 payload.

The per-item session parameters ``StreamInfo(K, nb, T, packet_tok)`` travel reliably out of band.  An item of T tokens is
P = ceil(T / packet_tok) packets; packet p carries tokens [p*packet_tok, min(T, (p+1)*packet_tok)).  One packet:

    offset  size  field
    0       2     magic  b"MP"
    2       1     version (1)
    3       4     seq      the packet number p                      (uint32, little-endian)
    7       1     ntok     tokens in this packet (packet_tok, less in the tail packet)
    8       1     nb_sent  books carried, 1..nb
    9       ...   nb_sent*ntok indices of ceil(log2 K) bits each, BOOK-major (all tokens of book 0, then book 1, ...), each index
                  least-significant bit first, bits packed LSB-first into bytes, the last byte zero-padded.

Book-major order makes a packet layered: dropping enhancement books is a truncation of the body (``thin``), no re-pack.  Residual
VQ is successively refinable, so a token that arrives with fewer books is a normal lower-rate token, not a loss.  At 8 books x
K = 512 x 2 tokens a body is 18 bytes.

``pack_bodies`` / ``unpack_bodies`` are the definition of the body layout; the device kernels (ops.idx_pack_packets /
ops.idx_unpack_packets) equal them bit for bit.  Bodies of one item form a regular array uint8[P, body_bytes(packet_tok, nb, K)]:
the shorter tail packet and every thinned packet are zero-padded to the full width.

The AUDIO codes travel in the same format (ProposedEval.compress_packets_av): StreamInfo(K = the DAC codebook size, nb = the stages
carried, T = the audio tokens, packet_tok), "books" being the stages of the DAC residual VQ, whose first m are a valid lower-rate
code.  Both streams share the magic ``MP`` and are told apart by the list they travel in; the format and ``VERSION`` do not change
(there is no stream-kind field).

FORWARD ERROR CORRECTION (``Fec``, fec_rows / frame_fec / gather_fec / fec_recover): one XOR parity packet, magic ``MF``, over the
first m books of every group of g data packets.  A body's first m books are a valid lower-rate body, so a packet rebuilt from the
parity is a packet thinned to m books: nothing downstream of ``fec_recover`` knows about it.  Parity packets travel in a list of
their own; the data packets, ``gather``, ``thin``, ``frame`` and ``VERSION`` are unchanged.  ``fec_rows`` / ``fec_recover`` are the
definition the device kernels (ops.fec_parity / ops.fec_recover) equal bit for bit.

``Fec(group, books, parity=r)``, r in 2..4: a systematic Reed-Solomon erasure code over GF(2^8) (polynomial 0x11d, generator 2)
with r parity packets per group.  Parity i has coefficient A[i][u] = 2^(i*u) for the group's packet u, so parity 0 is the XOR
packet above, byte for byte (magic ``MF``); parity i >= 1 travels with magic ``MR`` and one index byte behind the header.  Every
square submatrix of A (4 x 16) is nonsingular: any d deficient packets of a group come back from any d of its parity packets.

THE RECEIVER'S AUDIO OUTPUT (``AudioFade``): what the audio waveform does where audio tokens never arrived -- hold, fade to silence,
fade back in.  ``AudioFade.apply`` is the definition the device kernel (ops.audio_fade_) equals bit for bit.
"""
from __future__ import annotations

import dataclasses
import struct
from typing import Iterable, NamedTuple, Optional

import numpy as np

from .bitstream import index_bits

MAGIC = b"MP"
FEC_MAGIC = b"MF"                           # a parity packet (frame_fec); ``gather`` refuses it by its magic
FEC_RS_MAGIC = b"MR"                        # parity index i >= 1 of a Fec with parity > 1: the header, one byte i, then as ``MF``
FEC_MAX_GROUP = 16
FEC_MAX_PARITY = 4
VERSION = 1
_HEADER = struct.Struct("<2sBIBB")
HEADER_BYTES = _HEADER.size                 # 9
PACKET_TOK = 2                              # plc.PACKET_TOK (PLC/PLC1.py:68), restated so this module needs no torch


class StreamInfo(NamedTuple):
    """Session parameters of one item: codebook size, books, tokens, tokens per packet."""
    K: int
    nb: int
    T: int
    packet_tok: int = PACKET_TOK

    @property
    def P(self) -> int:
        return n_packets(self.T, self.packet_tok)

    def ntok(self, p: int) -> int:
        """Tokens packet p carries."""
        return max(0, min(self.packet_tok, self.T - p * self.packet_tok))


@dataclasses.dataclass(frozen=True)
class Rate:
    """Sender-side rate control (closed loop: the sender builds its AR history from exactly the books it sends, in the receiver's
    arithmetic; include/mvq.h, mvq_rvq_rate_f32).  Every packet carries at least ``min_books`` books.
      * neither ``tol2`` nor ``budget``: every packet carries all books in use;
      * ``tol2`` (fp32 > 0), constant quality: a token needs the fewest books m >= min_books that leave a residual energy
        E_m <= tol2 * E_0 (all of them when none does); a packet carries the max over its tokens;
      * ``budget`` (int), constant rate: the books of the 16 / packet_tok packets of a 16-token chunk sum to ``budget``, given out
        one at a time to the packet whose next book removes most residual energy (a shorter tail group of g packets gets
        max(g*min_books, budget*g // P_c)).
    ``tol2`` and ``budget`` are mutually exclusive (ValueError).  ``resolve`` checks the values against a stream's shape.
    ``beam`` (1..8; include/mvq.h, mvq_rvq_beam_f32): the sender searches the books with a beam of that many
    paths per token instead of greedily and sends the path with the smallest final residual -- the same bits on the wire, nothing
    changes at the receiver.  1: the greedy search, today's launches exactly.  The beam optimises the full depth: under ``tol2`` /
    ``budget`` / thinning a packet carries a PREFIX of the path, which is not the greedy prefix and may be worse than it."""
    min_books: int = 1
    tol2: Optional[float] = None
    budget: Optional[int] = None
    beam: int = 1

    def __post_init__(self):
        if self.tol2 is not None and self.budget is not None:
            raise ValueError("Rate: tol2 (constant quality) and budget (constant rate) are mutually exclusive")
        for name in ("min_books", "budget"):
            v = getattr(self, name)
            if v is not None and (isinstance(v, bool) or int(v) != v):
                raise ValueError(f"Rate: {name} = {v!r} is not an integer")
        if self.min_books < 1:
            raise ValueError(f"Rate: min_books = {self.min_books} (at least one book per packet: the format has no empty packet)")
        if isinstance(self.beam, bool) or not isinstance(self.beam, (int, np.integer)) or not 1 <= int(self.beam) <= 8:
            raise ValueError(f"Rate: beam = {self.beam!r} must be an integer in 1..8 (the slots the search keeps per token)")
        if self.tol2 is not None and not (np.float32(self.tol2) > 0 and np.isfinite(np.float32(self.tol2))):
            raise ValueError(f"Rate: tol2 = {self.tol2!r} must be a finite positive fp32 value")

    def __repr__(self):
        body = f"min_books={self.min_books!r}, tol2={self.tol2!r}, budget={self.budget!r}"
        return f"Rate({body})" if self.beam == 1 else f"Rate({body}, beam={self.beam!r})"

    def resolve(self, nb_use: int, packet_tok: int, group_tok: int = 16):
        """-> (min_books, mode, tol2, budget) as mvq_rvq_rate_f32 takes them (mode 0 full, 1 tol2, 2 budget); ValueError on a
        packet_tok that does not divide the chunk, min_books > nb_use, or a budget outside P_c*min_books .. P_c*nb_use."""
        nb_use, packet_tok, group_tok, min_books = int(nb_use), int(packet_tok), int(group_tok), int(self.min_books)
        if packet_tok < 1 or group_tok % packet_tok:
            raise ValueError(f"Rate: packet_tok = {packet_tok} does not divide the {group_tok}-token chunk")
        if nb_use > 0 and min_books > nb_use:
            raise ValueError(f"Rate: min_books = {min_books} outside 1..{nb_use} (the books in use)")
        if self.tol2 is not None:
            return min_books, 1, float(np.float32(self.tol2)), 0
        if self.budget is not None:
            budget, pc = int(self.budget), group_tok // packet_tok
            if nb_use > 0 and not pc * min_books <= budget <= pc * nb_use:
                raise ValueError(f"Rate: budget = {budget} outside {pc * min_books}..{pc * nb_use} "
                                 f"({pc} packets per chunk, {min_books}..{nb_use} books each)")
            return min_books, 2, 0.0, budget
        return min_books, 0, 0.0, 0


def sent_bits(nb_sent, info: StreamInfo, headers: bool = True) -> int:
    """Bits on the wire of one item whose packet p carries nb_sent[p] books (an int: every packet): the bodies as framed (whole
    bytes per packet), plus the 9-byte headers when ``headers``."""
    info = _check(info)
    counts = [int(nb_sent)] * info.P if np.ndim(nb_sent) == 0 else [int(v) for v in np.asarray(nb_sent).reshape(-1)]
    if len(counts) != info.P:
        raise ValueError(f"sent_bits: {len(counts)} counts for P={info.P} packets")
    return 8 * sum(body_bytes(info.ntok(p), counts[p], info.K) + (HEADER_BYTES if headers else 0) for p in range(info.P))


def sent_kbps(nb_sent, info: StreamInfo, headers: bool = True, token_rate: float = 75.0) -> float:
    """The realised rate of ``sent_bits`` in kbit/s at ``token_rate`` tokens per second (75: 24 kHz / 320)."""
    info = _check(info)
    return sent_bits(nb_sent, info, headers) * float(token_rate) / (1000.0 * info.T) if info.T else 0.0


def n_packets(t: int, packet_tok: int) -> int:
    return (int(t) + int(packet_tok) - 1) // int(packet_tok)


def body_bytes(ntok: int, nb: int, k: int) -> int:
    """Bytes of a body of ``nb`` books x ``ntok`` tokens: ceil(nb * ntok * ceil(log2 K) / 8)."""
    return (int(nb) * int(ntok) * index_bits(k) + 7) // 8


def _check(info: StreamInfo) -> StreamInfo:
    info = StreamInfo(*(int(v) for v in info))
    if info.K < 1 or not 0 <= info.nb <= 255 or info.T < 0 or not 1 <= info.packet_tok <= 255:
        raise ValueError(f"packets: {info} outside the format (K >= 1, nb <= 255, T >= 0, 1 <= packet_tok <= 255)")
    if info.P >= 2 ** 32:
        raise ValueError(f"packets: {info.P} packets do not fit the 32-bit sequence number")
    return info


def _pack_bits(vals, bits: int, nbytes: int) -> np.ndarray:
    """vals (element order) -> uint8[nbytes]: element e at bits [e*bits, (e+1)*bits), LSB first."""
    vals = np.asarray(vals, np.uint64).reshape(-1)
    planes = (vals[:, None] >> np.arange(bits, dtype=np.uint64)[None, :]) & np.uint64(1)
    out = np.zeros(nbytes, np.uint8)
    packed = np.packbits(planes.astype(np.uint8).reshape(-1), bitorder="little")
    out[:packed.size] = packed
    return out


def _unpack_bits(row, n: int, bits: int) -> np.ndarray:
    """The first n elements of a body row -> int64[n]."""
    if bits == 0 or n == 0:
        return np.zeros(n, np.int64)
    flat = np.unpackbits(np.asarray(row, np.uint8), bitorder="little")[:n * bits]
    return (flat.reshape(n, bits).astype(np.int64) << np.arange(bits, dtype=np.int64)[None, :]).sum(axis=1)


def pack_bodies(idx, info: StreamInfo) -> np.ndarray:
    """idx[nb, T] (integers in [0, K)) -> bodies uint8[P, body_bytes(packet_tok, nb, K)].  Raises ValueError on an index outside
    [0, K) (the device kernel clamps instead) or a shape that disagrees with ``info``."""
    info = _check(info)
    idx = np.asarray(idx)
    if idx.ndim != 2 or idx.shape != (info.nb, info.T):
        raise ValueError(f"pack_bodies: idx of shape {idx.shape} for nb={info.nb}, T={info.T}")
    if idx.size and not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"pack_bodies: integer indices expected, got {idx.dtype}")
    v = idx.astype(np.int64)
    if v.size and (v.min() < 0 or v.max() >= info.K):
        raise ValueError(f"pack_bodies: index outside [0, {info.K})")
    bits, full = index_bits(info.K), body_bytes(info.packet_tok, info.nb, info.K)
    out = np.zeros((info.P, full), np.uint8)
    for p in range(info.P):
        t0 = p * info.packet_tok
        out[p] = _pack_bits(v[:, t0:t0 + info.ntok(p)], bits, full)          # [nb, ntok] row-major = book-major
    return out


def unpack_bodies(bodies, nb_recv, info: StreamInfo):
    """bodies uint8[P, body_full], nb_recv[P] (books of each packet that arrived, 0 = lost; more than nb counts as nb)
    -> (idx[nb, T] int64, nb_valid[T] uint8).  Books at or above a packet's count decode as index 0 and are not counted in
    nb_valid; a value >= K (a corrupt body) is clamped to K-1, as the device kernel does."""
    info = _check(info)
    full = body_bytes(info.packet_tok, info.nb, info.K)
    bodies = np.asarray(bodies, np.uint8).reshape(-1, full) if full else np.zeros((info.P, 0), np.uint8)
    nb_recv = np.asarray(nb_recv).reshape(-1)
    if bodies.shape[0] != info.P or nb_recv.shape[0] != info.P:
        raise ValueError(f"unpack_bodies: {bodies.shape[0]} bodies / {nb_recv.shape[0]} counts for P={info.P} packets")
    bits = index_bits(info.K)
    idx = np.zeros((info.nb, info.T), np.int64)
    nb_valid = np.zeros(info.T, np.uint8)
    for p in range(info.P):
        t0, ntok = p * info.packet_tok, info.ntok(p)
        got = max(0, min(int(nb_recv[p]), info.nb))
        nb_valid[t0:t0 + ntok] = got
        vals = _unpack_bits(bodies[p], got * ntok, bits)
        idx[:got, t0:t0 + ntok] = np.minimum(vals, info.K - 1).reshape(got, ntok)
    return idx, nb_valid


def frame(bodies, info: StreamInfo, nb_sent=None, seq_base: int = 0) -> list:
    """bodies[P, body_full] -> one ``bytes`` per packet: the header and the first ``nb_sent`` (default: all nb) books of the body.
    ``nb_sent`` is one count for every packet or a sequence of P counts, one per packet (sender rate control): packet p then
    equals ``thin`` of the full packet to nb_sent[p] books.
    ``seq_base`` (streaming, stream.py): ``info`` describes one chunk of a longer stream and packet p is numbered seq_base + p,
    the stream's sequence number, as ``gather(seq_base=)`` expects it."""
    info = _check(info)
    seq_base = int(seq_base)
    if not 0 <= seq_base <= 2 ** 32 - info.P:
        raise ValueError(f"frame: seq_base = {seq_base} with P = {info.P} packets leaves the 32-bit sequence number")
    if nb_sent is None or np.ndim(nb_sent) == 0:
        counts = [info.nb if nb_sent is None else int(nb_sent)] * max(info.P, 1)
    else:
        counts = [int(v) for v in np.asarray(nb_sent).reshape(-1)]
        if len(counts) != info.P:
            raise ValueError(f"frame: {len(counts)} book counts for P={info.P} packets")
    for c in counts:
        if not 1 <= c <= info.nb:
            raise ValueError(f"frame: nb_sent={c} outside 1..{info.nb}")
    full = body_bytes(info.packet_tok, info.nb, info.K)
    bodies = np.asarray(bodies, np.uint8).reshape(-1, full) if full else np.zeros((info.P, 0), np.uint8)
    if bodies.shape[0] != info.P:
        raise ValueError(f"frame: {bodies.shape[0]} bodies for P={info.P} packets")
    out = []
    for p in range(info.P):
        ntok = info.ntok(p)
        out.append(_HEADER.pack(MAGIC, VERSION, seq_base + p, ntok, counts[p]) + _first_books(bodies[p], ntok, counts[p], info.K))
    return out


def _first_books(row, ntok: int, nb_keep: int, k: int) -> bytes:
    """The body of the first nb_keep books: a truncation, with the bits of the next book cleared from the last byte."""
    n = body_bytes(ntok, nb_keep, k)
    body = bytearray(np.asarray(row, np.uint8)[:n].tobytes())
    used = nb_keep * ntok * index_bits(k) - 8 * (n - 1)                      # bits of the last byte that belong to kept books
    if n and used < 8:
        body[-1] &= (1 << used) - 1
    return bytes(body)


def parse(packet, info: StreamInfo):
    """One packet -> (seq, nb_sent, body bytes); the ValueErrors of ``gather``."""
    return _parse(packet, _check(info))


def _parse(packet, info: StreamInfo, seq_base: int = 0):
    """``seq_base``: the sequence number of ``info``'s packet 0 (a chunk of a longer stream).  A packet from before it comes back
    as (negative seq, 0, b"") with only its magic and version checked: its chunk's shape is not ``info``'s."""
    data = bytes(packet)
    if len(data) < HEADER_BYTES:
        raise ValueError(f"packet: {len(data)} bytes, shorter than the {HEADER_BYTES}-byte header")
    magic, version, seq, ntok, nb_sent = _HEADER.unpack_from(data, 0)
    if magic != MAGIC:
        raise ValueError(f"packet: bad magic {magic!r}")
    if version != VERSION:
        raise ValueError(f"packet: unsupported version {version}")
    seq -= seq_base
    if seq < 0:
        return seq, 0, b""
    if seq >= info.P:
        raise ValueError(f"packet: seq {seq + seq_base} >= {seq_base} + P = {seq_base + info.P}")
    if ntok != info.ntok(seq):
        raise ValueError(f"packet {seq}: ntok {ntok}, the stream has {info.ntok(seq)} tokens there")
    if not 1 <= nb_sent <= info.nb:
        raise ValueError(f"packet {seq}: nb_sent {nb_sent} outside 1..{info.nb}")
    want = HEADER_BYTES + body_bytes(ntok, nb_sent, info.K)
    if len(data) != want:
        raise ValueError(f"packet {seq}: {len(data)} bytes, the header implies {want}")
    return seq, nb_sent, data[HEADER_BYTES:]


def thin(packet, nb_keep: int, info: StreamInfo) -> bytes:
    """The packet truncated to its first ``nb_keep`` books (what a congested relay forwards): equals packing those books afresh."""
    info = _check(info)
    seq, nb_sent, body = _parse(packet, info)
    nb_keep = int(nb_keep)
    if not 1 <= nb_keep <= nb_sent:
        raise ValueError(f"thin: nb_keep={nb_keep} outside 1..{nb_sent}")
    ntok = info.ntok(seq)
    return _HEADER.pack(MAGIC, VERSION, seq, ntok, nb_keep) + _first_books(np.frombuffer(body, np.uint8), ntok, nb_keep, info.K)


def gather(packets: Iterable, info: StreamInfo, seq_base: int = 0, late: Optional[list] = None):
    """Any iterable of received packets (missing, reordered, duplicated) -> (bodies uint8[P, body_full], nb_recv uint8[P]).
    Rows of packets that did not arrive stay zero with nb_recv = 0; of duplicates the one with more books is kept.  Raises
    ValueError on bad magic or version, seq >= P, an ntok that disagrees with ``info``, nb_sent outside 1..nb, or a body length
    that disagrees with the header.

    ``seq_base`` (streaming, stream.py): ``info`` describes one chunk of a longer stream whose packets carry the stream's sequence
    numbers seq_base .. seq_base + P - 1; row seq - seq_base takes the packet.  A number at or past seq_base + P raises as above.
    One below seq_base belongs to a chunk already decoded: it is appended to ``late`` when that is a list (and otherwise
    ignored), ValueError when ``late`` is None."""
    info = _check(info)
    seq_base = int(seq_base)
    if not 0 <= seq_base <= 2 ** 32 - info.P:
        raise ValueError(f"gather: seq_base = {seq_base} with P = {info.P} packets leaves the 32-bit sequence number")
    full = body_bytes(info.packet_tok, info.nb, info.K)
    buf, got = bytearray(info.P * full), bytearray(info.P)                   # plain byte buffers: no numpy call per packet
    for pkt in packets:
        seq, nb_sent, body = _parse(pkt, info, seq_base)
        if seq < 0:
            if late is None:
                raise ValueError(f"packet: seq {seq + seq_base} < seq_base = {seq_base}")
            late.append(pkt)
            continue
        if nb_sent > got[seq]:                                               # a richer copy is never shorter: it covers the poorer
            buf[seq * full:seq * full + len(body)] = body
            got[seq] = nb_sent
    return np.frombuffer(buf, np.uint8).reshape(info.P, full), np.frombuffer(got, np.uint8)


# ------------------------------------------------------------------------------------------------ forward error correction
def _gf_tables():
    """GF(2^8), polynomial x^8 + x^4 + x^3 + x^2 + 1 (0x11d), generator 2 -> (exp uint8[512] with exp[i] = 2^i, doubled so that
    exp[log a + log b] needs no modulo; log uint8[256], log[0] unused)."""
    exp, log, x = np.zeros(512, np.uint8), np.zeros(256, np.uint8), 1
    for i in range(255):
        exp[i], log[x] = x, i
        x = (x << 1) ^ (0x11d if x & 0x80 else 0)
    exp[255:510] = exp[:255]
    return exp, log


GF_EXP, GF_LOG = _gf_tables()


def gf_mul(a, b):
    """The GF(2^8) product, elementwise (scalars or uint8 arrays, broadcast)."""
    a, b = np.asarray(a, np.uint8), np.asarray(b, np.uint8)
    return np.where((a == 0) | (b == 0), np.uint8(0), GF_EXP[GF_LOG[a].astype(np.int64) + GF_LOG[b]])


def gf_inv(a: int) -> int:
    """The inverse of a nonzero field element."""
    if not 1 <= int(a) <= 255:
        raise ZeroDivisionError("gf_inv: 0 has no inverse")
    return int(GF_EXP[255 - int(GF_LOG[int(a)])])


def fec_coef(i: int, u: int) -> int:
    """A[i][u] = (2^u)^i: the coefficient of the group's packet u in parity i."""
    return int(GF_EXP[(int(i) * int(u)) % 255])


def gf_solve_matrix(idx, cols) -> np.ndarray:
    """The inverse of M[k][d] = A[idx[k]][cols[d]] (len(idx) == len(cols)) by Gauss-Jordan without pivoting: every leading minor
    of M is a square submatrix of A, none of which is singular."""
    d = len(cols)
    aug = [[fec_coef(i, q) for q in cols] + [int(k == e) for e in range(d)] for k, i in enumerate(idx)]
    for k in range(d):
        if aug[k][k] == 0:
            raise ZeroDivisionError("gf_solve_matrix: a zero pivot (indices outside the 4 x 16 code?)")
        inv = gf_inv(aug[k][k])
        aug[k] = [int(gf_mul(inv, v)) for v in aug[k]]
        for e in range(d):
            if e != k and aug[e][k]:
                f = aug[e][k]
                aug[e] = [v ^ int(gf_mul(f, w)) for v, w in zip(aug[e], aug[k])]
    return np.array([row[d:] for row in aug], np.uint8).reshape(d, d)


@dataclasses.dataclass(frozen=True, repr=False)
class Fec:
    """Parity over the first ``books`` books of every ``group`` consecutive packets; both ends know it out of band, like
    StreamInfo.  Parity group j covers packets [j*group, min(P, (j+1)*group)): G = ceil(P / group) groups per item.  Packet p,
    sent with nb_sent[p] books, is protected to c_p = min(books, nb_sent[p]) books: unequal error protection, the base books only.
    ``parity`` = r packets per group: 1 is the XOR packet; 2..4 a Reed-Solomon code over GF(2^8) whose parity 0 is that XOR packet
    and which recovers any d <= (arrived parity packets of the group) deficient packets.  ``resolve`` checks the values against a
    stream's shape."""
    group: int
    books: int
    parity: int = 1

    def __post_init__(self):
        for name in ("group", "books", "parity"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Fec: {name} = {v!r} is not an integer")

    def __repr__(self):
        return f"Fec(group={self.group!r}, books={self.books!r}" + (")" if self.parity == 1 else f", parity={self.parity!r})")

    @property
    def r(self) -> int:
        """The parity packets per group, validated: 1..4."""
        r = int(self.parity)
        if not 1 <= r <= FEC_MAX_PARITY:
            raise ValueError(f"Fec: parity = {r} outside 1..{FEC_MAX_PARITY}")
        return r

    def rows_shape(self, info: StreamInfo) -> tuple:
        """The shape of one item's parity rows: (G, g + W), with parity > 1 (G, r, g + W)."""
        g, _, G, W = self.resolve(info)
        return (G, g + W) if self.r == 1 else (G, self.r, g + W)

    def resolve(self, info: StreamInfo, chunk_tok: Optional[int] = None):
        """-> (g, m, G, W): the group size, the protected books, the groups per item and the width of the code field,
        body_bytes(packet_tok, m, K).  ValueError on group outside 1..16, books outside 1..nb, parity outside 1..4, K < 2 (bodies
        of no bits), and, with ``chunk_tok`` (the model's 16-token chunk), a group that does not divide the chunk_tok //
        packet_tok packets of a chunk: a group never straddles a chunk."""
        info = _check(info)
        g, m, _ = int(self.group), int(self.books), self.r
        if not 1 <= g <= FEC_MAX_GROUP:
            raise ValueError(f"Fec: group = {g} outside 1..{FEC_MAX_GROUP}")
        if not 1 <= m <= info.nb:
            raise ValueError(f"Fec: books = {m} outside 1..{info.nb} (the stream's books)")
        if info.K < 2:
            raise ValueError(f"Fec: K = {info.K}: bodies of no bits have nothing to protect")
        if chunk_tok is not None:
            chunk_tok = int(chunk_tok)
            if chunk_tok < 1 or chunk_tok % info.packet_tok or (chunk_tok // info.packet_tok) % g:
                raise ValueError(f"Fec: group = {g} does not divide the {chunk_tok} // {info.packet_tok} packets of a chunk")
        return g, m, (info.P + g - 1) // g, body_bytes(info.packet_tok, m, info.K)


def _fec_counts(nb_sent, info: StreamInfo, what: str) -> np.ndarray:
    if nb_sent is None or np.ndim(nb_sent) == 0:
        return np.full(info.P, info.nb if nb_sent is None else int(nb_sent), np.int64)
    counts = np.asarray(nb_sent).reshape(-1).astype(np.int64)
    if counts.shape[0] != info.P:
        raise ValueError(f"{what}: {counts.shape[0]} book counts for P={info.P} packets")
    return counts


def _fec_bodies(bodies, info: StreamInfo, what: str) -> np.ndarray:
    full = body_bytes(info.packet_tok, info.nb, info.K)
    bodies = np.asarray(bodies, np.uint8).reshape(-1, full) if full else np.zeros((info.P, 0), np.uint8)
    if bodies.shape[0] != info.P:
        raise ValueError(f"{what}: {bodies.shape[0]} bodies for P={info.P} packets")
    return bodies


def _prefix(row, ntok: int, c: int, k: int, width: int) -> np.ndarray:
    """prefix(p): the body of the first c books (``_first_books``: what ``thin`` to c books carries), zero-extended to width."""
    out = np.zeros(width, np.uint8)
    body = _first_books(row, ntok, c, k)
    out[:len(body)] = np.frombuffer(body, np.uint8)
    return out


def fec_rows(bodies, nb_sent, info: StreamInfo, fec: Fec) -> np.ndarray:
    """bodies[P, body_full], nb_sent (None or a scalar: every packet; or P counts) -> the item's parity uint8[G, g + W].
    Bytes 0..g-1 of row j: c_p = min(m, nb_sent[p]) of the group's packets (0 in the slots of a short tail group); bytes g..g+W-1:
    the XOR over the group's packets of prefix(p), the first body_bytes(ntok_p, c_p, K) bytes of row p with the bits of book c_p
    and above cleared in the last one, zero-extended to W.
    With fec.parity = r > 1 -> uint8[G, r, g + W]: row [j, i] carries the same count bytes, then the GF(2^8) sum over the group's
    packets u = p - j*g of A[i][u] * prefix(p); A[0][u] = 1, so row [j, 0] is the XOR row."""
    info = _check(info)
    g, m, G, W = fec.resolve(info)
    r = fec.r
    bodies, counts = _fec_bodies(bodies, info, "fec_rows"), _fec_counts(nb_sent, info, "fec_rows")
    if counts.size and (counts.min() < 0 or counts.max() > 255):
        raise ValueError("fec_rows: a book count outside 0..255")
    rows = np.zeros((G, r, g + W), np.uint8)
    for p in range(info.P):
        j, c = p // g, min(m, int(counts[p]))
        rows[j, :, p - j * g] = c
        prefix = _prefix(bodies[p], info.ntok(p), c, info.K, W)
        for i in range(r):
            rows[j, i, g:] ^= gf_mul(fec_coef(i, p - j * g), prefix)
    return rows.reshape(fec.rows_shape(info))


def _fec_group(info: StreamInfo, g: int, j: int) -> range:
    return range(j * g, min(info.P, (j + 1) * g))


def frame_fec(rows, info: StreamInfo, fec: Fec, seq_base: int = 0) -> list:
    """rows[G, g + W] (fec_rows) -> one ``bytes`` per group: the 9-byte header of the data packets with magic b"MF",
    seq = seq_base + j, the ``ntok`` byte holding the packets of the group g_j and the ``nb_sent`` byte max_p c_p; then the g_j count
    bytes; then the XOR bytes cut to max_p body_bytes(ntok_p, c_p, K) (everything past that is zero by construction).
    ``seq_base`` (streaming): ``info`` describes one chunk and group j is numbered seq_base + j, the stream's group number.
    With fec.parity = r > 1: rows[G, r, g + W] -> r packets per group, group-major.  Index 0 is the ``MF`` packet above, unchanged;
    index i >= 1 has magic b"MR", the same header fields, one byte i, then the count bytes and the code bytes cut the same way."""
    info = _check(info)
    g, m, G, W = fec.resolve(info)
    r = fec.r
    seq_base = int(seq_base)
    if not 0 <= seq_base <= 2 ** 32 - G:
        raise ValueError(f"frame_fec: seq_base = {seq_base} with G = {G} groups leaves the 32-bit sequence number")
    rows = np.asarray(rows, np.uint8).reshape(-1, r, g + W)
    if rows.shape[0] != G:
        raise ValueError(f"frame_fec: {rows.shape[0] * r} parity rows for G={G} groups of {r}")
    out = []
    for j in range(G):
        grp = _fec_group(info, g, j)
        for i in range(r):
            counts = [int(v) for v in rows[j, i, :len(grp)]]
            if any(not 1 <= c <= m for c in counts):
                raise ValueError(f"frame_fec: group {j}: a count outside 1..{m}")
            n = max(body_bytes(info.ntok(p), c, info.K) for p, c in zip(grp, counts))
            out.append(_HEADER.pack(FEC_RS_MAGIC if i else FEC_MAGIC, VERSION, seq_base + j, len(grp), max(counts))
                       + (bytes([i]) if i else b"") + rows[j, i, :len(grp)].tobytes() + rows[j, i, g:g + n].tobytes())
    return out


def gather_fec(fec_packets: Iterable, info: StreamInfo, fec: Fec, seq_base: int = 0, late: Optional[list] = None):
    """Any iterable of received parity packets -> (rows uint8[G, g + W], got uint8[G]).  Rows of groups whose parity did not arrive
    stay zero with got = 0; duplicates are harmless.  Raises ValueError as ``gather`` does: bad magic or version, a group number
    at or past seq_base + G, a g_j or a count that disagrees with ``info`` / ``fec``, a length that disagrees with the header and
    the counts.  ``seq_base`` / ``late`` as in ``gather``, in group numbers.
    With fec.parity = r > 1 -> (rows uint8[G, r, g + W], got uint8[G], a BITMASK: bit i set = parity i of the group arrived).
    ``MR`` packets are taken too (refused as a bad magic when r == 1); also refused: an index byte outside 1..r-1, and two parity
    packets of one group whose count bytes disagree."""
    info = _check(info)
    g, m, G, W = fec.resolve(info)
    r = fec.r
    seq_base = int(seq_base)
    if not 0 <= seq_base <= 2 ** 32 - G:
        raise ValueError(f"gather_fec: seq_base = {seq_base} with G = {G} groups leaves the 32-bit sequence number")
    rows, got = np.zeros((G, r, g + W), np.uint8), np.zeros(G, np.uint8)
    for pkt in fec_packets:
        data = bytes(pkt)
        if len(data) < HEADER_BYTES:
            raise ValueError(f"parity packet: {len(data)} bytes, shorter than the {HEADER_BYTES}-byte header")
        magic, version, seq, gj, cmax = _HEADER.unpack_from(data, 0)
        if magic != FEC_MAGIC and not (magic == FEC_RS_MAGIC and r > 1):
            raise ValueError(f"parity packet: bad magic {magic!r}")
        if version != VERSION:
            raise ValueError(f"parity packet: unsupported version {version}")
        i, head = 0, HEADER_BYTES                                            # the parity index; where the count bytes start
        if magic == FEC_RS_MAGIC:
            if len(data) < HEADER_BYTES + 1 or not 1 <= data[HEADER_BYTES] < r:
                raise ValueError(f"parity packet: parity index {list(data[HEADER_BYTES:HEADER_BYTES + 1])} outside 1..{r - 1}")
            i, head = data[HEADER_BYTES], HEADER_BYTES + 1
        j = seq - seq_base
        if j < 0:
            if late is None:
                raise ValueError(f"parity packet: seq {seq} < seq_base = {seq_base}")
            late.append(pkt)
            continue
        if j >= G:
            raise ValueError(f"parity packet: seq {seq} >= {seq_base} + G = {seq_base + G}")
        grp = _fec_group(info, g, j)
        if gj != len(grp):
            raise ValueError(f"parity packet {j}: covers {gj} packets, the stream has {len(grp)} there")
        if len(data) < head + gj:
            raise ValueError(f"parity packet {j}: {len(data)} bytes, shorter than its {gj} count bytes")
        counts = list(data[head:head + gj])
        if any(not 1 <= c <= m for c in counts) or max(counts) != cmax:
            raise ValueError(f"parity packet {j}: counts {counts} (header: {cmax}) outside 1..{m}")
        n = max(body_bytes(info.ntok(p), c, info.K) for p, c in zip(grp, counts))
        if len(data) != head + gj + n:
            raise ValueError(f"parity packet {j}: {len(data)} bytes, the header and counts imply {head + gj + n}")
        for k in range(r):
            if k != i and got[j] >> k & 1 and list(rows[j, k, :gj]) != counts:
                raise ValueError(f"parity packet {j}: counts {counts} of parity {i} disagree with parity {k}'s {list(rows[j, k, :gj])}")
        rows[j, i] = 0
        rows[j, i, :gj] = counts
        rows[j, i, g:g + n] = np.frombuffer(data, np.uint8, n, head + gj)
        got[j] |= 1 << i
    return rows.reshape(fec.rows_shape(info)), got


def fec_recover(bodies, nb_recv, rows, got, info: StreamInfo, fec: Fec):
    """THE recovery rule -> (bodies, nb_recv, recovered uint8[P]), copies.  For a group j whose parity arrived (got[j] != 0), with
    c_p = min(rows[j, p - j*g], m, nb): packet p is DEFICIENT when nb_recv[p] < c_p (lost, or thinned below its protected count).
    When exactly one packet q of the group is deficient, row q becomes (XOR bytes) ^ XOR_{p != q} prefix(p) over its first
    body_bytes(ntok_q, c_q, K) bytes and zero past them, nb_recv[q] = c_q, recovered[q] = 1: what ``thin`` of the sent packet to
    c_q books carries.  In every other case (no parity, nothing deficient, two or more deficient) the group stays as it arrived.

    With fec.parity = r > 1 (rows[G, r, g + W], got a bitmask of the arrived parity indices below r): the counts come from the
    lowest arrived index; with D the deficient packets and 1 <= |D| <= (arrived parities), the |D| LOWEST arrived indices i_k
    give, per byte, the syndromes S_k = parity_{i_k} ^ sum_{u not in D} A[i_k][u] * prefix(u); M x = S with M[k][d] = A[i_k][q_d]
    is solved and every q in D is rebuilt as above, all together.  With r == 1 this is the rule above word for word."""
    info = _check(info)
    g, m, G, W = fec.resolve(info)
    r = fec.r
    bodies = _fec_bodies(bodies, info, "fec_recover").copy()
    nb_recv = np.asarray(nb_recv, np.uint8).reshape(-1).copy()
    rows, got = np.asarray(rows, np.uint8).reshape(-1, r, g + W), np.asarray(got).reshape(-1)
    if nb_recv.shape[0] != info.P or rows.shape[0] != G or got.shape[0] != G:
        raise ValueError(f"fec_recover: {nb_recv.shape[0]} counts, {rows.shape[0] * r} parity rows, {got.shape[0]} flags for P={info.P}, "
                         f"G={G}, parity={r}")
    recovered = np.zeros(info.P, np.uint8)
    for j in range(G):
        arrived = ([0] if got[j] else []) if r == 1 else [i for i in range(r) if int(got[j]) >> i & 1]
        if not arrived:
            continue
        grp = _fec_group(info, g, j)
        c = {p: min(int(rows[j, arrived[0], p - j * g]), m, info.nb) for p in grp}
        deficient = [p for p in grp if int(nb_recv[p]) < c[p]]
        if not 1 <= len(deficient) <= len(arrived):
            continue
        use = arrived[:len(deficient)]
        syn = rows[j, use, g:].copy()                                        # [|D|, W]
        for p in grp:
            if p not in deficient:
                prefix = _prefix(bodies[p], info.ntok(p), c[p], info.K, W)
                for k, i in enumerate(use):
                    syn[k] ^= gf_mul(fec_coef(i, p - j * g), prefix)
        inv = gf_solve_matrix(use, [q - j * g for q in deficient])
        for d, q in enumerate(deficient):
            x = np.zeros(W, np.uint8)
            for k in range(len(use)):
                x ^= gf_mul(inv[d, k], syn[k])
            n = body_bytes(info.ntok(q), c[q], info.K)
            bodies[q] = 0
            bodies[q, :n] = x[:n]
            nb_recv[q], recovered[q] = c[q], 1
    return bodies, nb_recv, recovered


def fec_bits(info: StreamInfo, fec: Fec, nb_sent=None, headers: bool = True) -> int:
    """Bits on the wire of one item's parity packets as ``frame_fec`` cuts them (``sent_bits``'s counterpart): per group the XOR
    bytes, plus the 9-byte header and the count bytes when ``headers``; fec.parity = r such packets per group, those of index
    i >= 1 with their index byte."""
    info = _check(info)
    g, m, G, W = fec.resolve(info)
    r = fec.r
    counts = _fec_counts(nb_sent, info, "fec_bits")
    total = 0
    for j in range(G):
        grp = _fec_group(info, g, j)
        total += r * max(body_bytes(info.ntok(p), min(m, int(counts[p])), info.K) for p in grp) \
            + ((r * (HEADER_BYTES + len(grp)) + r - 1) if headers else 0)
    return 8 * total


def fec_kbps(info: StreamInfo, fec: Fec, nb_sent=None, headers: bool = True, token_rate: float = 75.0) -> float:
    """The rate of ``fec_bits`` in kbit/s at ``token_rate`` tokens per second: the overhead FEC adds to ``sent_kbps``."""
    info = _check(info)
    return fec_bits(info, fec, nb_sent, headers) * float(token_rate) / (1000.0 * info.T) if info.T else 0.0


# ------------------------------------------------------------------------- the receiver's audio output
AUDIO_HOP = 320                             # samples per audio token
AUDIO_TAIL = 8                              # the decoder gives 320*T - 8 samples for T tokens


@dataclasses.dataclass(frozen=True)
class AudioFade:
    """What the receiver's audio OUTPUT does with audio tokens that never arrived: the waveform is repeated for ``hold_tok`` = H
    tokens, fades to silence over ``fade_tok`` = F tokens, stays silent, and fades back in over one token when a token arrives.
    H >= 0, F >= 1, H + F <= 255.  ``apply`` is the definition the device kernel (ops.audio_fade_, mvq_audio_fade_f32) equals bit
    for bit.  With v[t] = "some stage of audio token t arrived" (na_valid[b, t] > 0):

        r[-1] = 0;  r[t] = 0 if v[t] else min(r[t-1] + 1, H + F)                          (integers)
        g[-1] = 1;  g[t] = 1.0f if r[t] <= H else float32(H + F - r[t]) / float32(F)      (one IEEE fp32 division)
        sample s of the 320*T - 8:  t = s // 320, j = s % 320
            w    = float32(j + 1) / float32(320)
            gain = g[t-1] + (g[t] - g[t-1]) * w        (three fp32 operations, each rounded, no fma)
            out[s] = +0 if gain == 0 else y[s] * gain

    Where g[t-1] == g[t] == 1 the gain is exactly 1 and the sample keeps its bits (-0 and a quiet NaN too).  Where the gain is 0 the
    result is +0 whatever y holds -- predicated, not multiplied, so junk decoded from a lost region (NaN, inf) reaches nothing.
    g never leaves [0, 1].  AudioFade(0, 1) is "mute with a one-token ramp", AudioFade(1, 4) "repeat once, fade over four tokens"."""
    hold_tok: int = 1
    fade_tok: int = 4

    def __post_init__(self):
        for name in ("hold_tok", "fade_tok"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"AudioFade: {name} = {v!r} is not an integer")
        if self.hold_tok < 0 or self.fade_tok < 1 or self.hold_tok + self.fade_tok > 255:
            raise ValueError(f"AudioFade: hold_tok = {self.hold_tok}, fade_tok = {self.fade_tok}; hold_tok >= 0, fade_tok >= 1 and "
                             "hold_tok + fade_tok <= 255")

    def runs(self, valid, r_prev: int = 0) -> np.ndarray:
        """r[t] of one item's ``valid`` [T] (nonzero = arrived), continuing a run of ``r_prev`` -> int64 [T]."""
        cap, r, out = int(self.hold_tok) + int(self.fade_tok), int(r_prev), []
        for v in np.asarray(valid).reshape(-1):
            r = 0 if v else min(r + 1, cap)
            out.append(r)
        return np.asarray(out, np.int64)

    def gains(self, r) -> np.ndarray:
        """g of the run lengths ``r`` -> float32, same shape."""
        r = np.asarray(r, np.int64)
        H, F = int(self.hold_tok), int(self.fade_tok)
        return np.where(r <= H, np.float32(1), (H + F - r).astype(np.float32) / np.float32(F)).astype(np.float32)

    def apply(self, y, valid) -> np.ndarray:
        """The faded waveform of y [B, 1, 320*T - 8] (or [B, 320*T - 8]) under valid [B, T] -> float32, y's shape."""
        y = np.asarray(y, np.float32)
        valid = np.asarray(valid)
        B, T = valid.shape
        flat = y.reshape(B, -1)
        if flat.shape[1] != max(0, AUDIO_HOP * T - AUDIO_TAIL):
            raise ValueError(f"AudioFade.apply: {flat.shape[1]} samples for {T} tokens ({AUDIO_HOP}*T - {AUDIO_TAIL})")
        out = np.empty_like(flat)
        s = np.arange(flat.shape[1])
        t, w = s // AUDIO_HOP, (s % AUDIO_HOP + 1).astype(np.float32) / np.float32(AUDIO_HOP)
        for b in range(B):
            g = np.concatenate([np.ones(1, np.float32), self.gains(self.runs(valid[b]))])      # g[-1] first
            g0, g1 = g[t], g[t + 1]
            gain = (g0 + ((g1 - g0) * w).astype(np.float32)).astype(np.float32)
            with np.errstate(invalid="ignore", over="ignore"):
                out[b] = np.where(gain == 0, np.float32(0), flat[b] * gain)
        return out.reshape(y.shape)


# ------------------------------------------------------- the loss pattern shared by training and the tools (csrc/channel.hip)
_U32 = 0xFFFFFFFF


@dataclasses.dataclass(frozen=True)
class Channel:
    """A lossy packet channel: a two-state Gilbert-Elliott chain per item over its packets (``p_gb`` good -> bad, ``p_bg`` bad ->
    good; p_gb = 0 is the i.i.d. channel).  A packet is lost with probability ``loss`` in the good state and ``loss_bad`` in the
    bad one; a surviving packet is thinned with probability ``thin`` to min_books .. nb-1 of its nb books.  ``seed`` selects the
    pattern; the draws are a stateless hash (channel_counts), so the same arguments give the same pattern on host and device."""
    loss: float = 0.0
    thin: float = 0.0
    min_books: int = 1
    p_gb: float = 0.0
    p_bg: float = 1.0
    loss_bad: float = 1.0
    seed: int = 0

    def __post_init__(self):
        for name in ("loss", "thin", "p_gb", "p_bg", "loss_bad"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)) or not 0.0 <= float(v) <= 1.0:
                raise ValueError(f"Channel: {name} = {v!r} is not a probability in [0, 1]")
        for name in ("min_books", "seed"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Channel: {name} = {v!r} is not an integer")
        if self.min_books < 1:
            raise ValueError(f"Channel: min_books = {self.min_books} (at least one book per surviving packet)")

    def thresholds(self):
        """(loss, thin, p_gb, p_bg, loss_bad) as 64-bit integers: an event of probability q happens when u < min(2**32, int(q * 2**32))."""
        return tuple(min(1 << 32, int(float(getattr(self, n)) * 4294967296.0)) for n in ("loss", "thin", "p_gb", "p_bg", "loss_bad"))


@dataclasses.dataclass(frozen=True)
class Link:
    """The link of a training step: the tactile stream's Channel, the audio stream's (None: the audio arrives whole) and the
    tokens per packet of both."""
    tactile: Channel
    audio: Optional[Channel] = None
    packet_tok: int = 2

    def __post_init__(self):
        if not isinstance(self.tactile, Channel) or not (self.audio is None or isinstance(self.audio, Channel)):
            raise ValueError("Link: tactile must be a Channel, audio a Channel or None")
        if isinstance(self.packet_tok, bool) or not isinstance(self.packet_tok, (int, np.integer)) or self.packet_tok < 1:
            raise ValueError(f"Link: packet_tok = {self.packet_tok!r} must be an integer >= 1")


def _chan_mix(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x7feb352d)
    x = x ^ (x >> np.uint32(15)); x = x * np.uint32(0x846ca68b)
    return x ^ (x >> np.uint32(16))


def _chan_fold(h, f):
    return _chan_mix((h ^ f) + np.uint32(0x9e3779b9))


def channel_counts(ch: Channel, nb: int, P: int, items: int, stream: int = 0, step: int = 0, item_base: int = 0) -> np.ndarray:
    """The definition of a Channel's pattern: uint8 [items, P], 0 = packet lost, otherwise the books (of ``nb``) that arrive.
    Pure uint32 / uint64 integer arithmetic on a stateless hash, every field taken mod 2**32:
        mix(x):     x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16
        fold(h, f) = mix((h ^ f) + 0x9e3779b9)
        u(draw)    = fold(fold(fold(fold(fold(fold(0, seed), step), stream), item_base + b), p), draw)
    An event of probability q happens when u < min(2**32, int(q * 2**32)) (Channel.thresholds).  Per item, from the good state:
        draw 0 moves the state before EVERY packet, packet 0 included (good -> bad on p_gb, bad -> good on p_bg);
        draw 1 loses the packet (``loss`` in the good state, ``loss_bad`` in the bad one): count 0;
        draw 2 thins a surviving packet (``thin``) when nb > min_books;
        draw 3 gives the books a thinned packet keeps: min_books + ((u * (nb - min_books)) >> 32), i.e. min_books .. nb-1.
    Row b depends on item_base + b alone: rows 0..5 of 256 items are the 6 items.  ops.channel_draw is this on the device."""
    nb, P, items = int(nb), int(P), int(items)
    if P < 0 or items < 0 or not 1 <= ch.min_books <= nb <= 255:
        raise ValueError(f"channel_counts: bad shape (items={items}, P={P}, min_books={ch.min_books}, nb={nb}; 1 <= min_books <= nb <= 255)")
    t_loss, t_thin, t_gb, t_bg, t_lbad = (np.uint64(t) for t in ch.thresholds())
    with np.errstate(over="ignore"):
        h = np.uint32(0)
        for f in (ch.seed, step, stream):
            h = _chan_fold(h, np.uint32(int(f) & _U32))
        item = ((np.arange(items, dtype=np.uint64) + np.uint64(int(item_base) & _U32)) & np.uint64(_U32)).astype(np.uint32)
        h_item = _chan_fold(np.full(items, h, dtype=np.uint32), item)
        out = np.zeros((items, P), dtype=np.uint8)
        bad = np.zeros(items, dtype=bool)
        span = np.uint64(nb - ch.min_books)
        for p in range(P):
            hp = _chan_fold(h_item, np.uint32(p))
            u = [_chan_fold(hp, np.uint32(d)).astype(np.uint64) for d in range(4)]
            bad = np.where(bad, ~(u[0] < t_bg), u[0] < t_gb)
            lost = u[1] < np.where(bad, t_lbad, t_loss)
            thinned = (u[2] < t_thin) & (nb > ch.min_books)
            kept = np.uint64(ch.min_books) + ((u[3] * span) >> np.uint64(32))
            out[:, p] = np.where(lost, 0, np.where(thinned, kept, nb)).astype(np.uint8)
    return out
