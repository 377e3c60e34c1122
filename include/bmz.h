/*
 * bmz.h -- C ABI of the MI355X BGZF block compressor ("bucket-map deflate", part of libbmf.so).
 *
 * The tools' output is text that every user converts to BAM next; that conversion is a single-threaded deflate of the
 * same bytes.  bmz_deflate turns a host buffer (a BAM stream) into BGZF blocks on the device, one workgroup per block.
 *
 * THE CONTRACT IS EXACT: a block's compressed bytes are a function of its input bytes alone -- not of the grid, of
 * scheduling, or of the other blocks of the call.  bucket-map_amd/host/bgzf.h states the same rule in C++ and
 * tests/bgzf_rule.py in Python; the three agree byte for byte.  The rule, in integers only:
 *
 * PARSE.  T = 256, HB = BMZ_HASH_BITS = 15, minimum match 4, maximum match 258, maximum distance 32 768.
 *   - Position i with i + 4 <= n has hash h(i) = (le32(b[i..i+4)) * 2654435761 mod 2^32) >> (32 - HB).
 *   - The block is taken in steps of T positions.  The candidate c(i) of a position in step s is the GREATEST position
 *     j < s*T with h(j) = h(i), or none: the table is read as it stood after the steps before s, and the positions of
 *     step s enter it after every lookup of that step.
 *   - L(i) = the common prefix of b[c..] and b[i..], capped at 258 and at n - i; 0 without a candidate or when
 *     i - c > 32 768.
 *   - Greedy walk from p = 0: L(p) >= 4 emits the match (L, p - c) and p += L; otherwise the literal b[p] and p += 1.
 *
 * CODES.  The deflate payload is whichever of stored (BTYPE 00), fixed Huffman (01), dynamic Huffman (10) has the fewest
 * BYTES; a tie goes to the earlier of the list.  One deflate block, BFINAL = 1.  The dynamic code lengths of an alphabet
 * (literal/length: 286 symbols with the end-of-block symbol counted once, limit 15; distance: 30 symbols, limit 15;
 * code-length: symbols 0..15 counted over the HLIT + HDIST lengths the header lists, limit 7; run codes 16/17/18 are
 * never used) come from its histogram f:
 *   - the m symbols with f > 0 in ascending (f, symbol) order are leaves 0..m-1;
 *   - m = 0 gives symbol 0 the length 1, m = 1 gives the one symbol the length 1 (the incomplete code inflate accepts);
 *   - otherwise m - 1 times: take the two lightest nodes, each from the head of the leaf queue or of the queue of made
 *     nodes (made nodes queue in the order they were made), a leaf winning an equal weight; make their parent;
 *   - count[l] = leaves at depth l, depths beyond the limit counted at the limit; K = sum count[l] * 2^(limit - l);
 *   - while K > 2^limit: take the greatest l < limit with count[l] > 0; count[l] -= 1, count[l+1] += 2,
 *     count[limit] -= 1, K -= 1   (so K ends at exactly 2^limit: the Kraft sum is 1);
 *   - lengths are dealt to the leaves in order 0..m-1, the longest first: count[limit] leaves get limit, and so on.
 *   Codes are canonical (RFC 1951 3.2.2).  HLIT, HDIST and HCLEN are the smallest that cover the non-zero lengths
 *   (HCLEN in the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, at least 4).
 *
 * WRAPPER.  1f 8b 08 04 00000000 00 ff 0600 'B' 'C' 0200 BSIZE(u16 = block length - 1), the payload, CRC32 (reflected
 * 0xEDB88320) and ISIZE, little-endian.  A block is at most n + 31 bytes (the stored form).
 *
 * Conventions as in bmv.h: plain C types, int status, message in bmz_last_error(), no CPU path.
 */
#ifndef BMZ_H
#define BMZ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMZ_OK = 0, BMZ_ERR_ARG = 1, BMZ_ERR_HIP = 2 };
enum { BMZ_BLOCK_MAX = 65280, BMZ_HASH_BITS = 15 };

typedef struct bmz_ctx bmz_ctx;

const char *bmz_last_error(void);
int  bmz_create(int32_t device, bmz_ctx **out);
void bmz_destroy(bmz_ctx *ctx);

/* Bytes `out` must hold for n_bytes cut into blocks of block_bytes: n + 31 per block.  0 for block_bytes = 0. */
uint64_t bmz_bound(uint64_t n_bytes, uint32_t block_bytes);

/* in[0, n_bytes) is cut into blocks of block_bytes (1 .. BMZ_BLOCK_MAX) by size alone, the last one may be shorter; every
 * block becomes one complete BGZF block, written back to back, in order, to out; *out_bytes = their total.  n_bytes = 0
 * succeeds and writes nothing (the caller appends the 28-byte EOF block itself).  block_bytes out of range or
 * out_cap < bmz_bound(n_bytes, block_bytes): BMZ_ERR_ARG, nothing ran, the context stays usable. */
int  bmz_deflate(bmz_ctx *ctx, const uint8_t *in, uint64_t n_bytes, uint32_t block_bytes, uint8_t *out, uint64_t out_cap,
                 uint64_t *out_bytes);

/* The last call's n_blocks + 1 offsets into out (out_offset[n_blocks] = *out_bytes). */
int  bmz_blocks(bmz_ctx *ctx, uint64_t *out_offset);

/* The last call's kernel time in ms (HIP events on the context's stream) and how many of its blocks took each form. */
int  bmz_last_stats(bmz_ctx *ctx, float *ms_kernels, uint32_t *n_stored, uint32_t *n_fixed, uint32_t *n_dynamic);

#ifdef __cplusplus
}
#endif
#endif
