"""A .bai reader and a region query over a BGZF file, standard library only (SAM spec 5.2, 5.3): what a viewer or a variant
caller does with x.bam + x.bam.bai.  A helper for tests/test_bamsort*.py, not a test module."""
import struct
import zlib

PSEUDO_BIN = 37450
BLOCK_MAX = 65280


def parse_bai(data):
    """{'refs': [{'bins': {bin: [(beg, end), ...]} in file order, 'bin_order': [...], 'pseudo': (first, end, n_mapped,
    n_unmapped) or None, 'linear': [...]}], 'n_no_coor': int}; the whole file must be consumed."""
    assert data[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<I", data, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<I", data, at)[0]
        at += 4
        bins, order, pseudo = {}, [], None
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<II", data, at)
            at += 8
            chunks = [struct.unpack_from("<QQ", data, at + 16 * k) for k in range(n_chunk)]
            at += 16 * n_chunk
            order.append(b)
            if b == PSEUDO_BIN:
                assert n_chunk == 2 and pseudo is None
                pseudo = (*chunks[0], *chunks[1])
            else:
                assert b not in bins and n_chunk >= 1
                bins[b] = chunks
        n_intv = struct.unpack_from("<I", data, at)[0]
        at += 4
        linear = list(struct.unpack_from(f"<{n_intv}Q", data, at))
        at += 8 * n_intv
        refs.append(dict(bins=bins, bin_order=order, pseudo=pseudo, linear=linear))
    n_no_coor = struct.unpack_from("<Q", data, at)[0]
    assert at + 8 == len(data)
    return dict(refs=refs, n_no_coor=n_no_coor)


def reg2bins(beg, end):
    """The bins that may hold a record overlapping [beg, end), 0-based half-open (SAM spec 5.3)."""
    end -= 1
    out = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(base + (beg >> shift), base + (end >> shift) + 1))
    return out


class Bgzf:
    """Random access by virtual offset; blocks are inflated on demand and kept."""

    def __init__(self, data):
        self.data = data
        self.cache = {}

    def block(self, at):
        if at not in self.cache:
            assert self.data[at: at + 4] == b"\x1f\x8b\x08\x04"
            size = struct.unpack_from("<H", self.data, at + 16)[0] + 1
            raw = zlib.decompress(self.data[at + 18: at + size - 8], -15)
            assert len(raw) == struct.unpack_from("<I", self.data, at + size - 4)[0]
            self.cache[at] = (raw, at + size)
        return self.cache[at]

    def read(self, voffset, n):
        """n bytes from the virtual offset on, and the virtual offset after them."""
        at, within = voffset >> 16, voffset & 0xFFFF
        out = b""
        while True:
            raw, nxt = self.block(at)
            take = raw[within: within + n - len(out)]
            out += take
            within += len(take)
            if raw and within == len(raw):
                at, within = nxt, 0
            if len(out) == n:
                return out, at << 16 | within
            assert raw, "read beyond the last block"


def record_span(rec):
    """(refID, beg, end, flag) of a record (with its block_size); end as the index counts it."""
    rid, pos, l_name, _mapq, _bin, n_cig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    ref_len = sum(c >> 4 for c in struct.unpack_from(f"<{n_cig}I", rec, 36 + l_name) if c & 15 in (0, 2, 3, 7, 8))
    beg = max(pos, 0)
    return rid, beg, max(pos + (ref_len or 1), beg + 1), flag


def normal(voffset, file):
    """A virtual offset at the very end of a block's data and one at the start of the next block name the same place."""
    at, within = voffset >> 16, voffset & 0xFFFF
    raw, nxt = file.block(at)
    return nxt << 16 if within == len(raw) and len(raw) else voffset


def fetch(bam, bai, ref, beg, end):
    """The records (bytes, with block_size) of reference `ref` that overlap [beg, end), found as the index allows: the chunks of
    the region's bins, without those that end at or before the linear index's offset for beg's window, read from each
    chunk's begin to its end."""
    index = parse_bai(bai) if isinstance(bai, (bytes, bytearray)) else bai
    file = bam if isinstance(bam, Bgzf) else Bgzf(bam)
    r = index["refs"][ref]
    w = beg >> 14
    floor = r["linear"][w] if w < len(r["linear"]) else (r["linear"][-1] if r["linear"] else 0)
    chunks = sorted(c for b in reg2bins(beg, end) for c in r["bins"].get(b, []) if c[1] > floor)
    out, seen = [], set()
    for c_beg, c_end in chunks:
        at, c_end = normal(c_beg, file), normal(c_end, file)
        while at < c_end:
            here = at
            head, at = file.read(at, 4)
            body, at = file.read(at, struct.unpack("<I", head)[0])
            rec = head + body
            rid, r_beg, r_end, _ = record_span(rec)
            assert rid == ref
            if r_beg < end and r_end > beg and here not in seen:
                seen.add(here)
                out.append(rec)
        assert at == c_end, "a chunk does not end on a record border"
    return out
