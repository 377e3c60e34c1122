"""Records for the coverage tests (tests/test_depth.py without a GPU, tests/test_depth_gpu.py with one): random records over
references whose lengths put scan tiles of 2 048 and reference borders everywhere relative to each other, and the edge list.
Every record satisfies what bmc_add checks (ops 0 .. 8, the CIGAR's query length is l_seq where there is a sequence)."""
import numpy as np

from test_markdup_gpu import OPS, rec, rec_ops

REF_LENS = [1, 2047, 2048, 2049, 4097, 70000]
SIZES = [0, 1, 2, 63, 64, 65, 257, 1025, 70001]
QUALS = np.array([0, 1, 14, 15, 40, 93, 254, 255], np.uint8)


def with_mapq(record, mapq):
    b = bytearray(record)
    b[13] = mapq
    return bytes(b)


def op(n, ch):
    return n << 4 | OPS.index(ch)


def query_len(ops):
    return sum(c >> 4 for c in ops if OPS[c & 15] in "MIS=X")


def random_ops(rng):
    """A CIGAR of 1 .. 12 ops: blocks of mostly short, sometimes long lengths with every other op between them."""
    ops = []
    if rng.random() < 0.2:
        ops.append(op(int(rng.integers(1, 4)), "H"))
    if rng.random() < 0.3:
        ops.append(op(int(rng.integers(1, 9)), "S"))
    for k in range(int(rng.integers(1, 5))):
        if k:
            ops.append(op(int(rng.integers(1, 30)), "DINP"[int(rng.integers(0, 4))]))
        n = int(rng.integers(1, 60)) if rng.random() < 0.9 else int(rng.integers(600, 3000))
        ops.append(op(n, "M=X"[int(rng.integers(0, 3))]))
        if rng.random() < 0.3:
            ops.append(op(int(rng.integers(1, 20)), "=X"[int(rng.integers(0, 2))]))      # an adjacent block
    if rng.random() < 0.3:
        ops.append(op(int(rng.integers(1, 9)), "S"))
    return ops


def random_records(n, seed, ref_len=REF_LENS):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(n):
        ref = int(rng.integers(0, len(ref_len)))
        if rng.random() < 0.5:
            ref = len(ref_len) - 1 - int(rng.integers(0, min(2, len(ref_len))))          # most on the longer ones
        length = ref_len[ref]
        how = rng.random()
        pos = int(rng.integers(0, length)) if how < 0.6 else max(0, length - 1 - int(rng.integers(0, 70))) if how < 0.9 else 0
        flag = 16 * int(rng.integers(0, 2)) | int(rng.choice([0, 0, 0, 0, 0, 0, 0x800, 1 | 0x40, 1 | 0x80, 4, 0x100, 0x200, 0x400]))
        ops = random_ops(rng)
        if rng.random() < 0.03:
            ops = []
        if rng.random() < 0.02:
            ref, pos = -1, -1
        l_seq = query_len(ops) if rng.random() < 0.8 or not ops else 0
        qual = QUALS[rng.integers(0, len(QUALS), l_seq)].tobytes() if ops else QUALS[rng.integers(0, 8, int(rng.integers(0, 9)))].tobytes()
        r = rec_ops(ref, pos, flag, ops, qual, b"q%d" % k, rng.bytes(int(rng.integers(0, 9))))
        out.append(with_mapq(r, int(rng.integers(0, 256))))
    return out


EDGE_REFS = [1000, 50, 1]


def edge_records():
    q = lambda n, first=20: bytes((first + k) % 200 for k in range(n))
    out = [
        rec(0, 990, 0, "10M", q(10), b"to_the_end"),                  # ends exactly at the end of the reference
        rec(0, 991, 0, "10M", q(10, 30), b"one_past"),                # 1 past it: clipped, its last quality too
        rec(0, 950, 16, "150M", q(150, 50), b"hundred_past"),
        rec(0, 999, 0, "5M", q(5, 90), b"last_base"),                 # pos == ref_len - 1
        rec(2, 0, 0, "3M", q(3, 7), b"on_one_base"),
        rec(0, 995, 0, "3M10D5M", q(8, 11), b"block_beyond"),         # the second block starts beyond the end: nothing of it
        rec(0, 996, 0, "2M2I4M", q(8, 60), b"insert_then_clip"),      # query bases 4 .. 5 count, 6 .. 7 do not
        rec(1, 50, 0, "5M", q(5), b"pos_is_len"),                     # not placed
        rec(1, -1, 0, "5M", q(5), b"pos_negative"),
        rec(-1, 5, 0, "5M", q(5), b"no_reference"),
        rec(0, 10, 0, "6S", q(6), b"clips_only"),                     # counted records without depth
        rec(0, 10, 0, "2H5S", q(5), b"hard_and_soft"),
        rec(0, 10, 0, "3P", b"", b"pads_only"),
        rec(0, 10, 0, "4I", q(4), b"insert_only"),
        rec(0, 10, 0, "", q(4), b"no_cigar"),                          # not placed
        rec(0, 20, 0, "5=1X4=", q(10), b"eq_x_eq"),                   # adjacent blocks: one run
        rec(0, 40, 0, "0M5M0X", q(5), b"empty_blocks"),
        rec(0, 100, 0, "10M", q(10), b"abut_a"), rec(0, 110, 0, "10M", q(10), b"abut_b"),              # one run
        rec(0, 200, 0, "10M", q(10), b"abut_c"), rec(0, 210, 0, "10M", q(10), b"abut_d"), rec(0, 210, 0, "10M", q(10), b"abut_e"),
        rec(0, 300, 0, "4M3D4M2N4M", q(12), b"gaps"),                 # D and N do not count
        rec(0, 400, 0, "8M", bytes([255] * 8), b"no_qualities"),      # 0xFF: neither sum nor count
        rec(0, 400, 0, "8M", bytes([255, 0, 255, 254, 1, 255, 255, 9]), b"some_qualities"),
        rec(0, 500, 0, "8M", b"", b"no_sequence"),                    # l_seq == 0
        rec_ops(1, 7, 0, [op(5, "S"), op(900, "N")], q(5), b"placeholder"),
        rec_ops(1, 7, 0, [op(5, "S"), op(900, "D")], q(5), b"no_placeholder"),
        rec_ops(1, 7, 0x400, [op(5, "S"), op(900, "N")], q(5), b"placeholder_dup"),    # not placed: no n_long either
    ]
    for flag in (0x4, 0x100, 0x200, 0x400, 0x800):
        out.append(rec(1, 10, flag, "5M", q(5), b"flag%x" % flag))
    for k in range(64):                                               # record lengths over every residue mod 16
        out.append(with_mapq(rec(1, k % 50, 0, "3S%dM" % (k + 1), bytes([15 + k % 70]) * (k + 4), b"e%d" % k, b"t" * (k % 5)), k))
    return out


def many_ops_record(ref, pos, with_sequence=True, n_ops=60000):
    """1=1X ... with D, I, N and P mixed in, between a hard and a soft clip."""
    body = [op(1 + k % 3, "=X=DX=I=XN=XP"[k % 13]) for k in range(n_ops - 4)]
    ops = [op(2, "H"), op(3, "S"), *body, op(4, "S"), op(1, "H")]
    assert len(ops) == n_ops
    rng = np.random.default_rng(n_ops)
    qual = rng.integers(0, 256, query_len(ops)).astype(np.uint8).tobytes() if with_sequence else b""
    return rec_ops(ref, pos, 0, ops, qual, b"many_ops", b"NMi" + bytes(4))


def parse_check_output(text):
    """(runs, stats, depth) of tests/cpp/depth_check.cpp's output."""
    lines = text.split("\n")
    n = int(lines[0].split()[1])
    runs = [tuple(int(x) for x in l.split()) for l in lines[1: 1 + n]]
    assert lines[1 + n] == "stats"
    rest = lines[2 + n:]
    n_ref = sum(1 for l in rest if l.startswith("depth"))
    stats = [[int(x) for x in l.split()] for l in rest[:n_ref]]
    depth = [[int(x) for x in l.split()[1:]] for l in rest[n_ref: 2 * n_ref]]
    return runs, stats, depth
