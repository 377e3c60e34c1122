"""The BGZF block rule of include/bmz.h, restated in plain Python (standard library only): parse, the three forms, the
length-limited code construction and the wrapper.  It shares no code with bucket-map_amd/host/bgzf.h or the kernels;
tests/test_bgzf.py checks it against gzip.decompress and the other two against it, byte for byte."""
import zlib

T, HB, MIN_MATCH, MAX_MATCH, MAX_DIST, BLOCK_MAX = 256, 15, 4, 258, 32768, 65280
EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def len_sym(length):
    s = 28
    while LEN_BASE[s] > length:
        s -= 1
    return s


def dist_sym(dist):
    s = 29
    while DIST_BASE[s] > dist:
        s -= 1
    return s


def hash4(b, i):
    return ((int.from_bytes(b[i:i + 4], "little") * 2654435761) & 0xFFFFFFFF) >> (32 - HB)


def parse(b):
    """Tokens of the block: an int is a literal, a pair is (length, distance)."""
    n = len(b)
    cand = [-1] * n
    table = {}
    for lo in range(0, n, T):
        hi = min(n, lo + T)
        hs = [hash4(b, i) if i + 4 <= n else -1 for i in range(lo, hi)]
        for i, h in zip(range(lo, hi), hs):
            if h >= 0:
                cand[i] = table.get(h, -1)
        for i, h in zip(range(lo, hi), hs):
            if h >= 0:
                table[h] = i                      # ascending i: the greatest stays
    tokens, p = [], 0
    while p < n:
        c, length = cand[p], 0
        if c >= 0 and p - c <= MAX_DIST:
            cap = min(MAX_MATCH, n - p)
            while length < cap and b[c + length] == b[p + length]:
                length += 1
        if length >= MIN_MATCH:
            tokens.append((length, p - c))
            p += length
        else:
            tokens.append(b[p])
            p += 1
    return tokens


def code_lengths(freq, max_bits):
    """The rule's code construction: see include/bmz.h."""
    lens = [0] * len(freq)
    order = sorted((i for i, f in enumerate(freq) if f > 0), key=lambda i: (freq[i], i))
    m = len(order)
    if m <= 1:
        lens[order[0] if m else 0] = 1
        return lens
    w = [freq[i] for i in order] + [0] * (m - 1)
    parent = [0] * (2 * m - 1)
    a, b, nxt = 0, m, m
    for _ in range(m - 1):
        pair = []
        for _ in range(2):
            if a < m and (b >= nxt or w[a] <= w[b]):
                pair.append(a)
                a += 1
            else:
                pair.append(b)
                b += 1
        w[nxt] = w[pair[0]] + w[pair[1]]
        parent[pair[0]] = parent[pair[1]] = nxt
        nxt += 1
    depth = [0] * (2 * m - 1)
    for node in range(2 * m - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    count = [0] * (max_bits + 1)
    for leaf in range(m):
        count[min(depth[leaf], max_bits)] += 1
    kraft = sum(count[l] << (max_bits - l) for l in range(1, max_bits + 1))
    while kraft > 1 << max_bits:
        bits = max_bits - 1
        while count[bits] == 0:
            bits -= 1
        count[bits] -= 1
        count[bits + 1] += 2
        count[max_bits] -= 1
        kraft -= 1
    at = 0
    for l in range(max_bits, 0, -1):
        for _ in range(count[l]):
            lens[order[at]] = l
            at += 1
    return lens


def canonical(lens):
    """RFC 1951 3.2.2: codes by length, then by symbol; returned bit-reversed, as they enter the stream."""
    max_len = max(lens)
    count = [0] * (max_len + 2)
    for l in lens:
        if l:
            count[l] += 1
    nxt, code = [0] * (max_len + 2), 0
    for l in range(1, max_len + 1):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = [0] * len(lens)
    for s, l in enumerate(lens):
        if l:
            c = nxt[l]
            nxt[l] += 1
            out[s] = int(format(c, f"0{l}b")[::-1], 2)
    return out


FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 30


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, bits):
        self.v |= value << self.n
        self.n += bits

    def bytes(self):
        return self.v.to_bytes((self.n + 7) // 8, "little")


def histograms(tokens):
    ll, d = [0] * 286, [0] * 30
    for t in tokens:
        if isinstance(t, tuple):
            ll[257 + len_sym(t[0])] += 1
            d[dist_sym(t[1])] += 1
        else:
            ll[t] += 1
    ll[256] += 1
    return ll, d


def body_bits(ll_freq, d_freq, ll_len, d_len):
    bits = sum(f * ll_len[s] for s, f in enumerate(ll_freq)) + sum(f * d_len[s] for s, f in enumerate(d_freq))
    bits += sum(ll_freq[257 + s] * LEN_EXTRA[s] for s in range(29)) + sum(d_freq[s] * DIST_EXTRA[s] for s in range(30))
    return bits


def dynamic_header(ll_len, d_len):
    """(hlit, hdist, hclen, cl_len, the code lengths the header lists)"""
    hlit = max(s for s in range(286) if ll_len[s]) + 1
    hdist = max(s for s in range(30) if d_len[s]) + 1
    listed = ll_len[:hlit] + d_len[:hdist]
    cl_freq = [0] * 19
    for l in listed:
        cl_freq[l] += 1
    cl_len = code_lengths(cl_freq, 7)
    hclen = max(k for k in range(19) if cl_len[CL_ORDER[k]]) + 1
    return hlit, hdist, max(hclen, 4), cl_len, listed


def put_tokens(w, tokens, ll_len, d_len):
    ll_code, d_code = canonical(ll_len), canonical(d_len)
    for t in tokens:
        if isinstance(t, tuple):
            s = len_sym(t[0])
            w.put(ll_code[257 + s], ll_len[257 + s])
            w.put(t[0] - LEN_BASE[s], LEN_EXTRA[s])
            s = dist_sym(t[1])
            w.put(d_code[s], d_len[s])
            w.put(t[1] - DIST_BASE[s], DIST_EXTRA[s])
        else:
            w.put(ll_code[t], ll_len[t])
    w.put(ll_code[256], ll_len[256])


def deflate_forms(b):
    """The three raw-deflate payloads of the block, [stored, fixed, dynamic], and the dynamic form's lengths."""
    n = len(b)
    tokens = parse(b)
    ll_freq, d_freq = histograms(tokens)
    stored = bytes([1]) + n.to_bytes(2, "little") + (n ^ 0xFFFF).to_bytes(2, "little") + bytes(b)
    w = Bits()
    w.put(1, 1)
    w.put(1, 2)
    put_tokens(w, tokens, FIXED_LL, FIXED_D)
    fixed = w.bytes()
    assert w.n == 3 + body_bits(ll_freq, d_freq, FIXED_LL, FIXED_D)
    ll_len, d_len = code_lengths(ll_freq, 15), code_lengths(d_freq, 15)
    hlit, hdist, hclen, cl_len, listed = dynamic_header(ll_len, d_len)
    cl_code = canonical(cl_len)
    w = Bits()
    w.put(1, 1)
    w.put(2, 2)
    w.put(hlit - 257, 5)
    w.put(hdist - 1, 5)
    w.put(hclen - 4, 4)
    for k in range(hclen):
        w.put(cl_len[CL_ORDER[k]], 3)
    for l in listed:
        w.put(cl_code[l], cl_len[l])
    put_tokens(w, tokens, ll_len, d_len)
    return [stored, fixed, w.bytes()], (ll_len, d_len, cl_len)


def deflate_block(b, only=None):
    """One complete BGZF block for b (at most BLOCK_MAX bytes) and the form it took (0 stored, 1 fixed, 2 dynamic): the
    smallest payload in bytes, a tie going to the earlier form.  `only` forces a form (size comparisons)."""
    assert len(b) <= BLOCK_MAX
    forms, _ = deflate_forms(b)
    form = min(range(3), key=lambda f: (len(forms[f]), f)) if only is None else only
    payload = forms[form]
    total = 18 + len(payload) + 8
    head = bytes.fromhex("1f8b08040000000000ff060042430200") + (total - 1).to_bytes(2, "little")
    return head + payload + zlib.crc32(b).to_bytes(4, "little") + len(b).to_bytes(4, "little"), form


def deflate(data, block_bytes=BLOCK_MAX):
    """bmz_deflate: (bytes, offsets of the n_blocks + 1 block starts, [n_stored, n_fixed, n_dynamic])"""
    out, offsets, forms = bytearray(), [0], [0, 0, 0]
    for at in range(0, len(data), block_bytes):
        blk, form = deflate_block(data[at:at + block_bytes])
        out += blk
        offsets.append(len(out))
        forms[form] += 1
    return bytes(out), offsets, forms
