"""CPU checker of the k-mer set's records and of its file (DESIGN.md "k-mer set file"; hypo_gpu_kset_export / _import, hypo --qv-save
/ --qv-load) in plain Python / numpy.  It shares no code with the library.

  mix64(x)                       the finaliser of MurmurHash3 on 64 bits
  home(key, slots)               the slot a key's probe starts at: (mix64(key) * slots) >> 64
  revcomp(key, k), canonical     the reverse complement of a 2k-bit code (A0 C1 G2 T3, MSB-first), and min(key, revcomp)
  record_digest / digest         mix64(key) + count * GOLD (mod 2^64), and the sum over a list (mod 2^64)
  write_file / file_bytes        the file of a list of blocks; parse_file: a strict parser, BadFile names the cause
  model(seqs, k)                 the set as a dict key -> count (stopping at 255) of read text, through qv_checker's windows
  merge(a, b)                    what importing b's records into a gives
"""
import struct

import numpy as np

import qv_checker as qc

M64 = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
MAGIC = b"HYPOKSET"
VERSION = 1


def mix64(x):
    x &= M64
    x ^= x >> 33
    x = (x * 0xFF51AFD7ED558CCD) & M64
    x ^= x >> 33
    x = (x * 0xC4CEB9FE1A85EC53) & M64
    x ^= x >> 33
    return x


def home(key, slots):
    return (mix64(key) * slots) >> 64


def revcomp(key, k):
    out = 0
    for _ in range(k):
        out = (out << 2) | (3 - (key & 3))
        key >>= 2
    return out


def canonical(key, k):
    return min(key, revcomp(key, k))


def record_digest(key, count):
    return (mix64(key) + count * GOLD) & M64


def digest(records):
    """records: an iterable of (key, count), or a dict"""
    items = records.items() if isinstance(records, dict) else records
    return sum(record_digest(int(k), int(c)) for k, c in items) & M64


def model(seqs, k, counting=True):
    """key -> min(255, windows of the sequences with that canonical code); counting=False: 1 for every key"""
    keys, n = np.unique(qc.canonical_windows(b"\n".join(bytes(s) for s in seqs), k), return_counts=True)      # (no window spans a newline)
    return {key: (min(255, c) if counting else 1) for key, c in zip(keys.tolist(), n.tolist())}


def merge(a, b):
    out = dict(a)
    for key, c in b.items():
        out[key] = min(255, out.get(key, 0) + c)
    return out


def file_bytes(k, blocks, n_keys=None, dig=None, version=VERSION, magic=MAGIC):
    """blocks: a list of lists of (key, count).  n_keys / dig: stated in the file in place of the true ones"""
    recs = [r for b in blocks for r in b]
    out = [magic, struct.pack("<IIQ", version, k, len(recs) if n_keys is None else n_keys)]
    for b in blocks:
        assert b, "a block holds at least one record"
        out.append(struct.pack("<Q", len(b)))
        out.append(struct.pack("<%dQ" % len(b), *[key for key, _ in b]))
        out.append(bytes(c for _, c in b))
        out.append(b"\0" * (-len(b) % 8))
    out.append(struct.pack("<QQ", 0, digest(recs) if dig is None else dig))
    return b"".join(out)


def write_file(path, k, blocks, **kw):
    with open(path, "wb") as f:
        f.write(file_bytes(k, blocks, **kw))


class BadFile(ValueError):
    """str(e) is one of CAUSES"""


CAUSES = ("bad magic", "bad version", "short read", "non-zero padding", "would pass n_keys", "below n_keys", "bytes after the digest")


def parse_bytes(data):
    """(k, n_keys, blocks as lists of (key, count), the digest the file states); refuses what DESIGN says a reader refuses"""
    at = [0]

    def take(n):
        if at[0] + n > len(data):
            raise BadFile("short read")
        at[0] += n
        return data[at[0] - n:at[0]]

    head = take(24)
    if head[:8] != MAGIC:
        raise BadFile("bad magic")
    version, k, n_keys = struct.unpack("<IIQ", head[8:])
    if version != VERSION:
        raise BadFile("bad version")
    blocks, total = [], 0
    while True:
        n, = struct.unpack("<Q", take(8))
        if n == 0:
            break
        if total + n > n_keys:
            raise BadFile("would pass n_keys")
        keys = struct.unpack("<%dQ" % n, take(8 * n))
        counts = take(n)
        if any(take(-n % 8)):
            raise BadFile("non-zero padding")
        blocks.append(list(zip(keys, counts)))
        total += n
    if total != n_keys:
        raise BadFile("below n_keys")
    dig, = struct.unpack("<Q", take(8))
    if at[0] != len(data):
        raise BadFile("bytes after the digest")
    return k, n_keys, blocks, dig


def parse_file(path):
    with open(path, "rb") as f:
        return parse_bytes(f.read())


def corrupted(k, blocks):
    """{cause: bytes of a file a reader must refuse for it}, made from a good file of `blocks` (at least two blocks, the first of
    them with a length that is no multiple of 8)"""
    good = file_bytes(k, blocks)
    n_recs = sum(len(b) for b in blocks)
    n0 = len(blocks[0])
    assert len(blocks) >= 2 and n0 % 8
    pad_at = 24 + 8 + 9 * n0                                             # the first padding byte of block 0
    return {
        "bad magic": b"HYPOKSEX" + good[8:],
        "bad version": file_bytes(k, blocks, version=2),
        "short read": good[:len(good) - 5],
        "short read in a block": good[:24 + 8 + 8 * n0 + 1],
        "short read in the header": good[:17],
        "non-zero padding": good[:pad_at] + b"\x01" + good[pad_at + 1:],
        "would pass n_keys": file_bytes(k, blocks, n_keys=n_recs - 1),
        "below n_keys": file_bytes(k, blocks, n_keys=n_recs + 1),
        "bytes after the digest": good + b"\0",
    }


def cause_of(name):
    """the member of CAUSES a key of corrupted() stands for"""
    return "short read" if name.startswith("short read") else name


def same_home(slot, slots, k, n, start=1):
    """the first n canonical k-mer codes from `start` upwards whose home slot in a table of `slots` slots is `slot`"""
    out, key = [], start
    while len(out) < n:
        if key <= revcomp(key, k) and home(key, slots) == slot:
            out.append(key)
        key += 1
    return out
