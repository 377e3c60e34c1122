"""Test helper for the BGZF inflater (include/bmu.h); no tests in it.

  inflate(raw)            a small pure-Python RFC 1951 decoder (standard library only; shares no code with
                          host/inflate_rule.h or the kernel): the bytes and a dict of what the stream used
  bgzf(...)               a BGZF writer around zlib's raw DEFLATE: cuts at given sizes, can inject Z_FULL_FLUSH
  literal_dynamic(...)    a literal-only dynamic block for given code lengths
  CASES                   name -> (BGZF bytes, the text they hold); CORRUPT: name -> (BGZF bytes, bad block, reason)
"""
import random
import struct
import zlib

import bgzf_rule as R

HEAD = bytes.fromhex("1f8b08040000000000ff060042430200")
EOF = R.EOF
(REASON_TRUNCATED, REASON_BLOCK_TYPE, REASON_STORED_LEN, REASON_CODE, REASON_DISTANCE, REASON_TOO_LONG, REASON_TOO_SHORT,
 REASON_CRC) = range(1, 9)


# ---- a pure-Python inflate ----
class _Bits:
    def __init__(self, raw):
        self.raw, self.at, self.acc, self.have = raw, 0, 0, 0

    def need(self, n):
        while self.have < n:
            if self.at >= len(self.raw):
                raise ValueError("truncated")
            self.acc |= self.raw[self.at] << self.have
            self.at += 1
            self.have += 8

    def get(self, n):
        if n == 0:
            return 0
        self.need(n)
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.have -= n
        return v


def _table(lens):
    """{(length, code read most significant bit first): symbol}"""
    codes = R.canonical(lens)
    return {(l, int(format(c, f"0{l}b")[::-1], 2)): s for s, (l, c) in enumerate(zip(lens, codes)) if l}


def _symbol(bits, table):
    code = 0
    for length in range(1, 16):
        code = code << 1 | bits.get(1)
        if (length, code) in table:
            return table[(length, code)]
    raise ValueError("no such code")


def inflate(raw):
    """(bytes, stats) of a raw DEFLATE stream."""
    st = dict(types=[], max_code_len=0, run_syms=set(), min_dist=None, max_dist=0, max_match=0, overlapping=0, empty_stored=0, one_dist_code=0)
    out = bytearray()
    bits = _Bits(raw)
    while True:
        final, btype = bits.get(1), bits.get(2)
        st["types"].append(btype)
        if btype == 0:
            bits.get(bits.have % 8)
            n, nn = bits.get(16), bits.get(16)
            assert n ^ 0xFFFF == nn and bits.have == 0
            st["empty_stored"] += n == 0
            out += raw[bits.at: bits.at + n]
            assert bits.at + n <= len(raw)
            bits.at += n
        else:
            assert btype in (1, 2)
            if btype == 1:
                ll_len, d_len = R.FIXED_LL, [5] * 32
            else:
                hlit, hdist, hclen = bits.get(5) + 257, bits.get(5) + 1, bits.get(4) + 4
                cl_len = [0] * 19
                for k in range(hclen):
                    cl_len[R.CL_ORDER[k]] = bits.get(3)
                cl = _table(cl_len)
                lens = []
                while len(lens) < hlit + hdist:
                    s = _symbol(bits, cl)
                    if s < 16:
                        lens.append(s)
                        continue
                    st["run_syms"].add(s)
                    if s == 16:
                        lens += [lens[-1]] * (3 + bits.get(2))
                    else:
                        lens += [0] * (3 + bits.get(3) if s == 17 else 11 + bits.get(7))
                assert len(lens) == hlit + hdist
                ll_len, d_len = lens[:hlit], lens[hlit:]
                st["max_code_len"] = max(st["max_code_len"], max(ll_len), max(d_len))
                st["one_dist_code"] += [l for l in d_len if l] == [1]
            ll, d = _table(ll_len), _table(d_len)
            while True:
                s = _symbol(bits, ll)
                if s < 256:
                    out.append(s)
                elif s == 256:
                    break
                else:
                    length = R.LEN_BASE[s - 257] + bits.get(R.LEN_EXTRA[s - 257])
                    ds = _symbol(bits, d)
                    dist = R.DIST_BASE[ds] + bits.get(R.DIST_EXTRA[ds])
                    assert dist <= len(out)
                    st["min_dist"] = dist if st["min_dist"] is None else min(st["min_dist"], dist)
                    st["max_dist"], st["max_match"] = max(st["max_dist"], dist), max(st["max_match"], length)
                    st["overlapping"] += length > dist
                    if dist >= length:
                        out += out[len(out) - dist: len(out) - dist + length]
                    else:
                        for _ in range(length):
                            out.append(out[-dist])
        if final:
            return bytes(out), st


# ---- writers ----
def wrap(raw, data, head=None):
    """One BGZF block around a raw DEFLATE payload; `head` replaces the 16 bytes before BSIZE (flags, extra subfields)."""
    if head is None:
        return HEAD + struct.pack("<H", 18 + len(raw) + 8 - 1) + raw + struct.pack("<II", zlib.crc32(data), len(data))
    total = len(head) + len(raw) + 8
    return head.replace(b"\xee\xee", struct.pack("<H", total - 1)) + raw + struct.pack("<II", zlib.crc32(data), len(data))


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), mem_level=9):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    out, at = b"", 0
    for p in flush_at:
        out += z.compress(data[at:p]) + z.flush(zlib.Z_FULL_FLUSH)
        at = p
    return out + z.compress(data[at:]) + z.flush()


def bgzf(data, sizes=65280, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=(), eof=True, mem_level=9):
    """`data` as BGZF: cut every `sizes` bytes (an int) or at the sizes of a list (the rest in blocks of the last one).
    Returns (bytes, in_offset, out_offset), the offsets with n_blocks + 1 entries each, the EOF block counted."""
    sizes = [sizes] if isinstance(sizes, int) else list(sizes)
    out, in_off, out_off, at, k = bytearray(), [0], [0], 0, 0
    while at < len(data):
        n = sizes[min(k, len(sizes) - 1)]
        piece = data[at: at + n]
        out += wrap(raw_deflate(piece, level, strategy, flush_at if k == 0 else (), mem_level), piece)
        at += len(piece)
        k += 1
        in_off.append(len(out))
        out_off.append(at)
    if eof:
        out += EOF
        in_off.append(len(out))
        out_off.append(at)
    return bytes(out), in_off, out_off


def literal_dynamic(lens, data):
    """A raw DEFLATE stream of one dynamic block that codes `data` (bytes below len(lens) - 1) as literals: the literal code
    lengths are lens[:-1], the end-of-block symbol takes lens[-1], everything else 0; one distance length of 0."""
    ll = list(lens[:-1]) + [0] * (256 - len(lens) + 1) + [lens[-1]]
    listed = ll + [0]
    cl_freq = [0] * 19
    for l in listed:
        cl_freq[l] += 1
    cl_len = R.code_lengths(cl_freq, 7)
    cl_code, ll_code = R.canonical(cl_len), R.canonical(ll)
    hclen = max(k for k in range(19) if cl_len[R.CL_ORDER[k]]) + 1
    w = R.Bits()
    w.put(1, 1)
    w.put(2, 2)
    w.put(0, 5)
    w.put(0, 5)
    w.put(max(hclen, 4) - 4, 4)
    for k in range(max(hclen, 4)):
        w.put(cl_len[R.CL_ORDER[k]], 3)
    for l in listed:
        w.put(cl_code[l], cl_len[l])
    for b in data:
        w.put(ll_code[b], ll[b])
    w.put(ll_code[256], ll[256])
    return w.bytes()


QUALS = [chr(33 + q) for q in range(39)]                    # 39 quality values, most of them near 30
QUAL_WEIGHTS = [2.0 ** (-abs(q - 30) / 4) for q in range(39)]


def fastq(n_bytes, seed=5):
    """Synthetic FASTQ text of 150-bp reads."""
    rng = random.Random(seed)
    out, i, have = [], 0, 0
    while have < n_bytes:
        seq = "".join(rng.choices("ACGT", k=150))
        qual = "".join(rng.choices(QUALS, weights=QUAL_WEIGHTS, k=150))
        out.append(f"@read{i} sample:{rng.randrange(10 ** 6)}\n{seq}\n+\n{qual}\n")
        have += len(out[-1])
        i += 1
    return "".join(out).encode()[:n_bytes]


def payload(block):
    """The raw DEFLATE payload of one plain-header BGZF block."""
    return block[18: len(block) - 8]


# ---- the cases ----
OVERSIZE = []       # (test_bgzf case, form) left out: see _make_cases


def _make_cases():
    from test_bgzf import CASES as BGZF_CASES
    c = {}
    for name, data in BGZF_CASES.items():
        forms = R.deflate_forms(data)[0]                # what R.deflate_block(data, only=form) wraps, parsed once
        for form in range(3):
            if 18 + len(forms[form]) + 8 > 65536:       # BSIZE is 16 bits: incompressible bytes in a Huffman form are no block
                OVERSIZE.append((name, form))
                continue
            c[f"rule_{name}_form{form}"] = (wrap(forms[form], data), data)
    rng = random.Random(77)
    c["z6_zeros"] = bytes(65280)
    c["z6_acg"] = b"ACG" * 20000
    for period in (2, 63, 64, 65):
        c[f"z6_period{period}"] = (rng.randbytes(period) * (65000 // period + 1))[:65000]
    c["z6_fastq"] = fastq(63000)
    c["z6_random"] = rng.randbytes(65280)
    for name in list(c):
        if name.startswith("z6_"):
            # memLevel 8 (zlib's default, what bgzip writes) ends a block after 16 383 symbols: the FASTQ member holds two
            c[name] = (bgzf(c[name], eof=False, mem_level=8 if name == "z6_fastq" else 9)[0], c[name])
    text = b"the quick brown fox jumps over the lazy dog, " * 8
    c["zfixed"] = (bgzf(text, strategy=zlib.Z_FIXED, eof=False)[0], text)
    fq = fastq(63000)
    c["z1_fastq"] = (bgzf(fq, level=1, eof=False)[0], fq)
    rep = (b"GATTACA-" * 40 + b"\n") * 41
    rep = rep[:13000]
    c["flushes"] = (bgzf(rep, flush_at=(100, 100, 7000), eof=False)[0], rep)
    data = bytes(rng.choices(range(15), weights=[2 ** (14 - i) for i in range(15)], k=3000)) + bytes(range(15))
    c["deep_literals"] = (wrap(literal_dynamic(list(range(1, 16)) + [15], data), data), data)
    head = bytes.fromhex("1f8b080c0000000000ff") + struct.pack("<H", 4 + 3 + 6) + b"XY\x03\x00abc" + b"BC\x02\x00\xee\xee" + b"reads.fq\x00"
    c["fname_extra"] = (wrap(raw_deflate(text), text, head), text)
    return c


def _make_corrupt(cases):
    """name -> (BGZF bytes, bad block, reason): each derived from a small valid case."""
    text = b"the quick brown fox jumps over the lazy dog, " * 8
    raw = raw_deflate(text)
    k = {}
    k["cut_short"] = (wrap(raw[: len(raw) // 2], text), 0, REASON_TRUNCATED)
    k["block_type_3"] = (wrap(bytes([raw[0] | 6]) + raw[1:], text), 0, REASON_BLOCK_TYPE)
    stored = bytearray(R.deflate_forms(text)[0][0])
    stored[3] ^= 1
    k["stored_nlen"] = (wrap(bytes(stored), text), 0, REASON_STORED_LEN)
    # a dynamic header whose code-length code is oversubscribed: HCLEN = 4 and four code-length codes of length 1
    w = R.Bits()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(0, 4)
    for _ in range(4):
        w.put(1, 3)
    w.put(0, 64)
    k["oversubscribed"] = (wrap(w.bytes(), text), 0, REASON_CODE)
    # ... and one whose literal/length lengths oversubscribe: three codes of length 1
    ll = [1, 1, 1] + [0] * 253 + [2]
    k["oversubscribed_ll"] = (wrap(_dynamic_header_only(ll), text), 0, REASON_CODE)
    # a first match with distance 1 at output position 0 (fixed code: length 3 = symbol 257 = 0000001, distance 1 = 00000)
    w = R.Bits()
    w.put(1, 1), w.put(1, 2)
    w.put(int("0000001"[::-1], 2), 7), w.put(0, 5)
    w.put(0, 7)
    k["distance_at_0"] = (wrap(w.bytes(), b"aaa"), 0, REASON_DISTANCE)
    good = wrap(raw, text)
    k["isize_less"] = (good[:-4] + struct.pack("<I", len(text) - 1), 0, REASON_TOO_LONG)
    k["isize_more"] = (good[:-4] + struct.pack("<I", len(text) + 1), 0, REASON_TOO_SHORT)
    crc = bytearray(good)
    crc[-8] ^= 0x10
    k["crc_bit"] = (bytes(crc), 0, REASON_CRC)
    # the bad block is not the first: valid blocks around it
    k["third_block"] = (good + EOF + k["crc_bit"][0] + good + EOF, 2, REASON_CRC)
    return k


def _dynamic_header_only(ll):
    listed = ll + [0]
    cl_freq = [0] * 19
    for l in listed:
        cl_freq[l] += 1
    cl_len = R.code_lengths(cl_freq, 7)
    cl_code = R.canonical(cl_len)
    hclen = max(4, max(i for i in range(19) if cl_len[R.CL_ORDER[i]]) + 1)
    w = R.Bits()
    w.put(1, 1), w.put(2, 2), w.put(0, 5), w.put(0, 5), w.put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl_len[R.CL_ORDER[i]], 3)
    for l in listed:
        w.put(cl_code[l], cl_len[l])
    w.put(0, 64)
    return w.bytes()


def format_errors():
    """name -> bytes that are not BGZF framing (BMU_ERR_FORMAT)."""
    import gzip
    text = b"the quick brown fox jumps over the lazy dog, " * 8
    good = wrap(raw_deflate(text), text)
    bsize_far = bytearray(good)
    struct.pack_into("<H", bsize_far, 16, len(good) + 10)
    big = bytearray(good)
    struct.pack_into("<I", big, len(big) - 4, 65537)
    no_room = HEAD + struct.pack("<H", 18 + 4 - 1) + b"\0\0\0\0"
    return {
        "plain_gzip": gzip.compress(text),
        "text": b"@read\nACGT\n+\nIIII\n" * 3,
        "trailing": good + b"junk after the last member",
        "short_tail": good + good[:10],
        "cm": good[:2] + b"\x07" + good[3:],
        "bsize_beyond": bytes(bsize_far),
        "isize_big": bytes(big),
        "no_trailer_room": no_room,
        "extra_overrun": good[:10] + struct.pack("<H", 6) + b"BC\x09\x00" + good[16:],
    }


CASES = _make_cases()
CORRUPT = _make_corrupt(CASES)
