/*
 * bms.h -- C ABI of the MI355X BAM record sorter ("bucket-map sort", part of libbmf.so).
 *
 * The tools' BAM stream (-o x.bam) is uploaded whole for bmz_deflate; with --sort its records are put in coordinate order
 * on the device between the upload and the deflate, so a sorted, indexable file costs no second pass over the bytes.
 *
 * THE ORDER IS EXACT, in integers only:
 *   - A record is rec_offset[i] .. rec_offset[i + 1] of the stream: block_size (u32), then block_size bytes, of which the
 *     first eight are refID (i32) and pos (i32), little-endian -- the record's bytes 4..12.
 *   - key(i) = (uint64)(uint32)refID << 32 | (uint32)(pos + 1).  So refID = -1 (unplaced) sorts last and pos = -1 sorts
 *     before pos = 0.
 *   - perm is the permutation with key(perm[0]) <= key(perm[1]) <= ..., and perm[a] < perm[b] wherever a < b have equal
 *     keys: records of equal key keep the order they came in (a stable sort).  That is Python's
 *     sorted(range(n), key=lambda i: (key[i], i)).
 *   - sorted_offset[0] = 0, sorted_offset[k + 1] = sorted_offset[k] + length(perm[k]); the sorted stream holds record
 *     perm[k] at sorted_offset[k].
 *   The result is a function of the input alone: not of the grid, of scheduling, or of the context's history.
 *   bucket-map_amd/host/bgzf.h (block_compressor::sort_records) states the same rule with std::stable_sort.
 *
 * bms_sort_deflate sorts, then cuts the sorted stream into blocks by size alone and deflates them as bmz_deflate does
 * (include/bmz.h: the same bytes as bmz_deflate of the sorted stream), without the stream leaving the device.
 *
 * ARGUMENT CHECKS run on the host before any device work.  Each of these returns BMS_ERR_ARG, runs nothing and leaves the
 * context usable: rec_offset[0] != 0; offsets not strictly ascending; rec_offset[n_records] != n_bytes; a record shorter
 * than 36 bytes (block_size and the 32 fixed bytes) or longer than 2^32 - 1; a record whose block_size field is not its
 * extent - 4; n_records > 2^31 - 1; block_bytes outside 1 .. BMZ_BLOCK_MAX; out_cap < bmz_bound(n_bytes, block_bytes);
 * a null pointer (in / out_sorted / out may be null when n_bytes = 0, out_perm when n_records = 0).  The context is looked
 * at last, so the checks of the data need no device.  n_records = 0 succeeds (sorted_offset[0] = 0, no bytes).  A failed
 * allocation returns BMS_ERR_HIP with the sizes in the message.
 *
 * Conventions as in bmz.h: plain C types, int status, message in bms_last_error(), no CPU path.
 */
#ifndef BMS_H
#define BMS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BMS_OK = 0, BMS_ERR_ARG = 1, BMS_ERR_HIP = 2 };
enum { BMS_MIN_RECORD = 36 };

typedef struct bms_ctx bms_ctx;

const char *bms_last_error(void);
int  bms_create(int32_t device, bms_ctx **out);
void bms_destroy(bms_ctx *ctx);

/* The n_records records of in[0, n_bytes) in key order: out_sorted[0, n_bytes) the sorted stream, out_perm[n_records],
 * out_sorted_offset[n_records + 1]. */
int  bms_sort(bms_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records,
              uint8_t *out_sorted, uint32_t *out_perm, uint64_t *out_sorted_offset);

/* The same sort; out receives the BGZF blocks of the sorted stream (block_bytes, out_cap, *out_bytes as in bmz_deflate). */
int  bms_sort_deflate(bms_ctx *ctx, const uint8_t *in, uint64_t n_bytes, const uint64_t *rec_offset, uint64_t n_records,
                      uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes, uint32_t *out_perm,
                      uint64_t *out_sorted_offset);

/* The last call's kernel times in ms (HIP events on the context's stream): keys + histogram + the radix passes, the gather
 * (lengths, their scan, the copy), the deflate (0 after bms_sort); and the number of radix passes that ran (0 .. 8). */
int  bms_last_stats(bms_ctx *ctx, float *ms_sort, float *ms_gather, float *ms_deflate, uint32_t *n_passes);

#ifdef __cplusplus
}
#endif
#endif
