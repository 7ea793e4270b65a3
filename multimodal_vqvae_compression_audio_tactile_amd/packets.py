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
"""
from __future__ import annotations

import dataclasses
import struct
from typing import Iterable, NamedTuple, Optional

import numpy as np

from .bitstream import index_bits

MAGIC = b"MP"
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
    ``tol2`` and ``budget`` are mutually exclusive (ValueError).  ``resolve`` checks the values against a stream's shape."""
    min_books: int = 1
    tol2: Optional[float] = None
    budget: Optional[int] = None

    def __post_init__(self):
        if self.tol2 is not None and self.budget is not None:
            raise ValueError("Rate: tol2 (constant quality) and budget (constant rate) are mutually exclusive")
        for name in ("min_books", "budget"):
            v = getattr(self, name)
            if v is not None and (isinstance(v, bool) or int(v) != v):
                raise ValueError(f"Rate: {name} = {v!r} is not an integer")
        if self.min_books < 1:
            raise ValueError(f"Rate: min_books = {self.min_books} (at least one book per packet: the format has no empty packet)")
        if self.tol2 is not None and not (np.float32(self.tol2) > 0 and np.isfinite(np.float32(self.tol2))):
            raise ValueError(f"Rate: tol2 = {self.tol2!r} must be a finite positive fp32 value")

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
