/*
 * bmu.h -- C ABI of the MI355X BGZF block inflater ("bucket-map unzip", part of libbmf.so): the reading side of bmz.h.
 *
 * FASTQ and FASTA files are practically always compressed.  BGZF (bgzip, htslib, bmz_deflate) is gzip cut into independent
 * members of at most 64 KiB, each with its size in its header, so a device can inflate all blocks of a file at once:
 * bmu_inflate turns a host buffer of whole BGZF blocks into their text, one wavefront per block
 * (bucket-map_amd/csrc/bmu_kernels.hip.h).  The decoder is a full RFC 1951 inflate -- stored, fixed and dynamic blocks in
 * any mix, several per member, codes up to 15 bits, run symbols 16/17/18, distances up to 32 768, overlapping matches, the
 * one-symbol distance code -- not only what bmz_deflate emits.  bucket-map_amd/host/bgzf_in.h restates it serially on the
 * host from the same lines (host/inflate_rule.h).
 *
 * FRAMING (RFC 1952), decided on the host without a device: magic 1f 8b, CM 8, FEXTRA set; the BC subfield of length 2
 * holds BSIZE = member length - 1 and is found by walking the subfields; FNAME, FCOMMENT and FHCRC are skipped;
 * BSIZE + 1 must reach a trailer inside the buffer; ISIZE <= 65536.  Empty blocks are legal anywhere.  Plain gzip (a
 * member without BC) is one serial stream and is refused: BMU_ERR_FORMAT with the offset and a hint at bgzip.
 *
 * Conventions as in bmz.h: plain C types, int status, message in bmu_last_error(), a context per device, no CPU path.
 */
#ifndef BMU_H
#define BMU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* BMU_ERR_FORMAT: the bytes are not BGZF framing.  BMU_ERR_DATA: the framing is fine, a block's payload is invalid or
 * does not match its CRC32 or ISIZE (bmu_bad_block tells which and why). */
enum { BMU_OK = 0, BMU_ERR_ARG = 1, BMU_ERR_HIP = 2, BMU_ERR_FORMAT = 3, BMU_ERR_DATA = 4 };

enum {
    BMU_REASON_NONE = 0,
    BMU_REASON_TRUNCATED = 1,      /* the stream needs bits beyond the block's payload */
    BMU_REASON_BLOCK_TYPE = 2,     /* BTYPE 11 */
    BMU_REASON_STORED_LEN = 3,     /* LEN != ~NLEN */
    BMU_REASON_CODE = 4,           /* oversubscribed or otherwise invalid code */
    BMU_REASON_DISTANCE = 5,       /* distance beyond the start of the block */
    BMU_REASON_TOO_LONG = 6,       /* output longer than ISIZE */
    BMU_REASON_TOO_SHORT = 7,      /* output shorter than ISIZE */
    BMU_REASON_CRC = 8             /* CRC32 mismatch */
};

typedef struct bmu_ctx bmu_ctx;

const char *bmu_last_error(void);

/* Host only, no context, no device.  The blocks of in[0, n_bytes): in_offset[i] = where block i starts in `in`,
 * out_offset[i] = where its text starts; both hold *n_blocks + 1 entries (the last ones are n_bytes and *out_bytes).
 * Null arrays: the counts only.  Anything that is not BGZF framing, trailing bytes included: BMU_ERR_FORMAT. */
int  bmu_layout(const uint8_t *in, uint64_t n_bytes, uint64_t *in_offset, uint64_t *out_offset, uint64_t *n_blocks,
                uint64_t *out_bytes);

int  bmu_create(int32_t device, bmu_ctx **out);
void bmu_destroy(bmu_ctx *ctx);

/* in[0, n_bytes) holds whole BGZF blocks; their text goes to out back to back, *out_bytes = its length (the layout's
 * total).  out_cap below that total: BMU_ERR_ARG, nothing ran.  BMU_ERR_DATA: nothing of out is promised; the context
 * stays usable. */
int  bmu_inflate(bmu_ctx *ctx, const uint8_t *in, uint64_t n_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_bytes);

/* The first bad block of the last bmu_inflate and its BMU_REASON_*; block = UINT64_MAX and reason 0 when there was none. */
int  bmu_bad_block(bmu_ctx *ctx, uint64_t *block, uint32_t *reason);

/* The last call's kernel time in ms (HIP events on the context's stream) and how many DEFLATE blocks (not BGZF blocks)
 * of each type it decoded. */
int  bmu_last_stats(bmu_ctx *ctx, float *ms_kernels, uint64_t *n_stored, uint64_t *n_fixed, uint64_t *n_dynamic);

#ifdef __cplusplus
}
#endif
#endif
