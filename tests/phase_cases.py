"""Calls and records for the phasing tests (tests/test_phase.py without a GPU, tests/test_phase_gpu.py with one): het calls
planted over pileup_cases' random records, chains of H linked sites, and the small designed cases of the rule.  A call is the 24
words of bmg_call; the phasing rule reads words 0, 1, 3, 4 and 5 only."""
import numpy as np

from pileup_cases import LETTER_CODES, Sample, rec_letters

VARIANT_FLAGS = 3


def het(ref, pos, a0=0, a1=1, R=None):
    return (ref, pos, a0 if R is None else R, VARIANT_FLAGS, a0, a1) + (0,) * 18


def hom(ref, pos, a=1):
    return (ref, pos, 0, VARIANT_FLAGS, a, a) + (0,) * 18


def no_variant(ref, pos):
    return (ref, pos, 0, 1, 0, 1) + (0,) * 18            # two letters, but not VARIANT: no phase site


def planted_calls(ref_len, bases, seed, gap=6):
    """Het calls every 1 .. 2 gap - 1 bases over every reference: allele 0 or 1 (at random) is the letter most reads carry
    there (pileup_cases.Sample, as random_records cuts its reads), the other allele another letter; one site in ten has two
    random letters.  Hom calls and calls that are no variant lie between them and are no phase sites."""
    rng = np.random.default_rng(seed)
    out = []
    for r, (n, b) in enumerate(zip(ref_len, bases)):
        codes = Sample(b, 1000 + r).codes
        p = int(rng.integers(0, gap))
        while p < n:
            kind = rng.random()
            if kind < 0.1:
                out.append(hom(r, p, int(rng.integers(0, 4))))
            elif kind < 0.2:
                out.append(no_variant(r, p))
            else:
                at = np.flatnonzero(LETTER_CODES == codes[p])
                mine = int(at[0]) if at.size and rng.random() < 0.9 else int(rng.integers(0, 4))
                other = (mine + 1 + int(rng.integers(0, 3))) % 4
                out.append(het(r, p, mine, other, R=int(rng.integers(0, 4))) if rng.random() < 0.5 else het(r, p, other, mine, R=mine))
            p += int(rng.integers(1, 2 * gap))
    return out


def chain(H, seed, bridged=False, spacing=3):
    """(records, ref_len, calls, haps): H sites at positions 1, 1 + spacing, ... of one reference, alleles A and C, and a
    hidden haplotype haps[k] (which allele haplotype 1 carries).  Every two neighbours are linked by two reads of two sites, one
    from either haplotype: one fully linked chain at d = 1.  bridged: the neighbours k, k + 1 with odd k get one read that
    agrees with the haplotypes and one that does not, a tie, and every even k is linked to k + 2 by two reads that show no letter
    (N) at k + 1: the chain runs at d = 2 over every odd link."""
    rng = np.random.default_rng(seed)
    haps = rng.integers(0, 2, H).tolist()
    ref_len = [spacing * max(H, 1) + 2]
    calls = [het(0, 1 + spacing * k) for k in range(H)]
    letter = lambda k, h: "AC"[haps[k] ^ h]
    recs = []
    for k in range(H - 1):
        tie = bridged and k % 2 == 1
        for h in (0, 1):
            second = letter(k + 1, h ^ 1) if tie and h else letter(k + 1, h)
            recs.append(rec_letters(0, 1 + spacing * k, f"{spacing + 1}M", letter(k, h) + "G" * (spacing - 1) + second, name=b"n%d_%d" % (k, h)))
        if bridged and k % 2 == 0 and k + 2 < H:
            for h in (0, 1):
                seq = letter(k, h) + "G" * (spacing - 1) + "N" + "G" * (spacing - 1) + letter(k + 2, h)
                recs.append(rec_letters(0, 1 + spacing * k, f"{2 * spacing + 1}M", seq, name=b"b%d_%d" % (k, h)))
    order = rng.permutation(len(recs)).tolist()
    return [recs[i] for i in order], ref_len, calls, haps


def reads_over(sites_letters, times=1, ref=0, name=b"d", **kw):
    """Records of len(letters) bases at position 0 of `ref`, [(letters, times)]: a designed case puts its sites at consecutive
    positions and spells what every read shows at each ('N': nothing)."""
    return [rec_letters(ref, 0, f"{len(letters)}M", letters, name=name + b"%d_%d" % (i, k), **kw)
            for i, (letters, n) in enumerate(sites_letters) for k in range(n * times)]


# ---- the designed cases of the rule, worked out by hand ----
# Each takes `rule(reads, calls, ref_len=(16,), **params) -> (link, words, sums)`: link an (H, reach, 4) array, words the 8 words
# of every site as tuples, sums the four sums; it raises phase_rule.Refused where the engine refuses.  The tests hand in the
# engine under test (host/phase.h through its checker, the device through a context), so the values below pin that engine.
def case_false_het_in_the_middle(rule):
    """Three sites at 0, 1, 2.  Both haplotypes show either allele at the middle one equally often: its two links tie; the link
    of the outer two at d = 2 is all cis.  The middle site is bridged and is itself a root."""
    import phase_rule as K
    calls = [het(0, 0), het(0, 1), het(0, 2)]
    link, words, sums = rule(reads_over([("AAA", 2), ("ACA", 2), ("CAC", 2), ("CCC", 2)]), calls)
    assert link[0, 0].tolist() == [2, 2, 2, 2] and link[1, 0].tolist() == [2, 2, 2, 2] and link[0, 1].tolist() == [4, 0, 0, 4]
    assert words == [(0, 0, 0, 0, K.PHASED | K.ROOT, 0, 0, 0), (1, 1, 1, 0, K.ROOT, 0, 0, 0), (2, 0, 0, 0, K.PHASED, 2, 8, 0)]
    assert sums == [3, 2, 1, 24]                         # the blocks interleave: site 1 lies inside the block of 0 and 2


def case_tie_min_links_and_min_frac_at_their_bounds(rule):
    import phase_rule as K
    import pytest
    calls = [het(0, 0), het(0, 1)]
    tie = reads_over([("AA", 3), ("AC", 3)])
    assert rule(tie, calls)[1][1][K.W_FLAGS] == K.ROOT and rule(tie, calls, min_frac_ppm=500001)[1][1][K.W_FLAGS] == K.ROOT
    assert rule(tie, calls, min_frac_ppm=500001, min_links=1)[1][1] == (1, 1, 1, 0, K.ROOT, 0, 0, 0)
    two = reads_over([("AC", 1), ("CA", 1)])             # trans wins with 2 links
    assert rule(two, calls)[1][1] == (1, 0, 0, 1, K.PHASED, 1, 0, 2)
    assert rule(two, calls, min_links=3)[1][1][K.W_FLAGS] == K.ROOT and rule(two[:1], calls)[1][1][K.W_FLAGS] == K.ROOT   # one short
    assert rule(two[:1], calls, min_links=1)[1][1][K.W_FLAGS] == K.PHASED
    four_to_one = reads_over([("AA", 4), ("AC", 1)])     # 4 x 1 000 000 == 800 000 x 5: exactly met, and one below
    assert rule(four_to_one, calls, min_frac_ppm=800000)[1][1] == (1, 0, 0, 0, K.PHASED, 1, 4, 1)
    assert rule(four_to_one, calls, min_frac_ppm=800001)[1][1][K.W_FLAGS] == K.ROOT
    one_to_four = reads_over([("AC", 4), ("CC", 1)])     # the same with trans as the larger side
    assert rule(one_to_four, calls, min_frac_ppm=800000)[1][1] == (1, 0, 0, 1, K.PHASED, 1, 1, 4)
    assert rule(one_to_four, calls, min_frac_ppm=800001)[1][1][K.W_FLAGS] == K.ROOT
    for bad in (dict(min_frac_ppm=500000), dict(min_frac_ppm=1000001), dict(min_links=0), dict(reach=0), dict(reach=9)):
        with pytest.raises(K.Refused):
            rule(two, calls, **bad)


def case_two_alternative_letters_and_what_is_no_observation(rule):
    import phase_rule as K
    calls = [het(0, 0, 1, 2, R=0), hom(0, 1), het(0, 2, 0, 3), no_variant(0, 3), het(0, 4, 3, 1, R=3)]
    reads = reads_over([("CATAT", 2), ("GAAAC", 2), ("AATAT", 5), ("CANAC", 1)])      # A at the 1/2 het: a third letter
    reads += reads_over([("CATAT", 3)], qual=[40, 40, 12, 40, 255], name=b"q")         # quality 12 at site 1, 0xFF at site 2
    link, words, sums = rule(reads, calls)
    assert [w[0] for w in words] == [0, 2, 4]            # the index of the call among the calls given
    assert link[0, 0].tolist() == [0, 2, 2, 0] and link[1, 0].tolist() == [0, 2, 2 + 5, 0] and link[0, 1].tolist() == [2 + 3, 1, 0, 2]
    # both links at d = 1 are all trans; the link at d = 2 (cis 7, trans 1) is never asked: the smallest d comes first
    assert [w[K.W_HAP] for w in words] == [0, 1, 0] and sums[:3] == [3, 3, 1] and sums[3] == 6 + 6 + 10 + 2 + 6
    assert words[1] == (2, 0, 0, 1, K.PHASED, 1, 0, 4) and words[2] == (4, 0, 0, 0, K.PHASED, 1, 0, 9) and words[0][K.W_FLAGS] == K.PHASED | K.ROOT
    quals = rule(reads_over([("CATAT", 3)], qual=[40, 40, 13, 40, 12], name=b"q"), calls)   # 13 counts under min_bq 13, 12 does not
    assert quals[0][0, 0].tolist() == [0, 3, 0, 0] and not quals[0][1].any() and not quals[0][0, 1].any() and quals[2][3] == 6


def case_blocks_interleave_and_reach_one_against_eight(rule):
    import phase_rule as K
    import pytest
    calls = [het(0, p) for p in range(10)]
    reads = reads_over([("ANANANANAN", 2), ("CNCNCNCNCN", 2), ("NANCNANCNA", 2), ("NCNANCNANC", 2)])
    link, words, sums = rule(reads, calls, reach=2)
    assert [w[K.W_ROOT] for w in words] == [0, 1] * 5 and [w[K.W_ROOT_POS] for w in words] == [0, 1] * 5 and sums[:3] == [10, 10, 2]
    assert [w[K.W_HAP] for w in words] == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0] and all(w[K.W_D] == 2 for w in words[2:])
    assert rule(reads, calls, reach=1)[2][:3] == [10, 0, 0]
    far = reads_over([("ANNNNNNNA", 2), ("CNNNNNNNC", 2)])       # sites 0 and 8 only
    assert rule(far, calls[:9], reach=8)[1][8] == (8, 0, 0, 0, K.PHASED, 8, 4, 0) and rule(far, calls[:9], reach=7)[2][:3] == [9, 0, 0]
    near = reads_over([("ANNNA", 2), ("CNNNC", 2)])              # sites 0 and 4: reach 4 reaches, reach 3 does not
    assert rule(near, calls[:5], reach=4)[1][4] == (4, 0, 0, 0, K.PHASED, 4, 4, 0) and rule(near, calls[:5], reach=3)[2][:3] == [5, 0, 0]
    with pytest.raises(K.Refused):                       # the calls ascend
        rule(far, [het(0, 3), het(0, 3)])
    with pytest.raises(K.Refused):
        rule(far, [het(0, 16)])
    with pytest.raises(K.Refused):
        rule(far, [het(0, 3, 4, 1)])


DESIGNED = [case_false_het_in_the_middle, case_tie_min_links_and_min_frac_at_their_bounds, case_two_alternative_letters_and_what_is_no_observation,
            case_blocks_interleave_and_reach_one_against_eight]
