"""Byte format of the transmitted codes (host side, numpy): one payload per item and code kind.

The reference states its rate as ``kbps = tps * books * log2(K)`` (Evaluation/dac_vcpwq_proposed6_latency.py:725-727): every
index costs exactly ceil(log2 K) bits.  A payload is that, behind a 15-byte header:

    offset  size  field
    0       4     magic  b"MVQI"
    4       1     version (1)
    5       2     nb     number of books / code rows        (uint16, little-endian)
    7       4     K      codebook size, 1 <= K < 2**32       (uint32, little-endian)
    11      4     T      tokens                              (uint32, little-endian)
    15      ...   T*nb indices of ceil(log2 K) bits each, token-major (all books of token 0, then token 1, ...), each index
                  least-significant bit first, bits packed LSB-first into bytes, the last byte zero-padded.

At 8 books x K = 512 a second of signal (75 tokens) is 5400 bits = 675 bytes of payload.  There is no entropy coding.
"""
from __future__ import annotations

import struct

import numpy as np

MAGIC = b"MVQI"
VERSION = 1
_HEADER = struct.Struct("<4sBHII")
HEADER_BYTES = _HEADER.size                 # 15


def index_bits(k: int) -> int:
    """ceil(log2 K): the bits one index takes (0 when K == 1)."""
    return (int(k) - 1).bit_length()


def payload_bits(nb: int, t: int, k: int) -> int:
    """Bits of the index payload, before the pad to a byte."""
    return int(nb) * int(t) * index_bits(k)


def pack_indices(idx, k: int) -> bytes:
    """idx[nb, T] (integers in [0, K)) -> bytes.  Raises ValueError on an index outside [0, K) or a shape the header cannot hold."""
    idx = np.asarray(idx)
    k = int(k)
    if idx.ndim != 2:
        raise ValueError(f"pack_indices: idx must be [n_books, T], got shape {idx.shape}")
    if idx.size and not np.issubdtype(idx.dtype, np.integer):
        raise ValueError(f"pack_indices: integer indices expected, got {idx.dtype}")
    nb, t = idx.shape
    if not 1 <= k < 2 ** 32 or nb >= 2 ** 16 or t >= 2 ** 32:
        raise ValueError(f"pack_indices: K={k}, nb={nb}, T={t} outside the header's range")
    v = idx.astype(np.int64)
    if v.size and (v.min() < 0 or v.max() >= k):
        raise ValueError(f"pack_indices: index outside [0, {k})")
    bits = index_bits(k)
    vals = np.ascontiguousarray(v.T).reshape(-1).astype(np.uint64)          # token-major
    planes = (vals[:, None] >> np.arange(bits, dtype=np.uint64)[None, :]) & np.uint64(1)
    body = np.packbits(planes.astype(np.uint8).reshape(-1), bitorder="little").tobytes()
    return _HEADER.pack(MAGIC, VERSION, nb, k, t) + body


def unpack_indices(payload) -> tuple[np.ndarray, int]:
    """bytes -> (idx[nb, T] int64, K).  Raises ValueError on a wrong magic or version, a length that does not match the
    header (truncated or trailing bytes) or an index >= K."""
    data = bytes(payload)
    if len(data) < HEADER_BYTES:
        raise ValueError(f"unpack_indices: {len(data)} bytes, shorter than the {HEADER_BYTES}-byte header")
    magic, version, nb, k, t = _HEADER.unpack_from(data, 0)
    if magic != MAGIC:
        raise ValueError(f"unpack_indices: bad magic {magic!r}")
    if version != VERSION:
        raise ValueError(f"unpack_indices: unsupported version {version}")
    if k < 1:
        raise ValueError("unpack_indices: K = 0")
    bits = index_bits(k)
    nbits = payload_bits(nb, t, k)
    want = HEADER_BYTES + (nbits + 7) // 8
    if len(data) != want:
        raise ValueError(f"unpack_indices: {len(data)} bytes, the header implies {want}" +
                         (" (truncated)" if len(data) < want else ""))
    flat = np.unpackbits(np.frombuffer(data, np.uint8, offset=HEADER_BYTES), bitorder="little")[:nbits]
    planes = flat.reshape(nb * t, bits).astype(np.int64)
    vals = (planes << np.arange(bits, dtype=np.int64)[None, :]).sum(axis=1) if bits else np.zeros(nb * t, np.int64)
    if vals.size and vals.max() >= k:
        raise ValueError(f"unpack_indices: index {int(vals.max())} >= K = {k}")
    return np.ascontiguousarray(vals.reshape(t, nb).T), int(k)
