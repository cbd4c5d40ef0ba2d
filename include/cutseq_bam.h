/*
 * cutseq_bam.h -- one BAM record -> one four-line FASTQ record: the decisions host and device must agree on.
 *
 * Plain C that gcc compiles into the host library (csh_bam_walk, cutseq_amd/csrc/cutseq_host.c) and into
 * tools/bam_walk_check.c (under the sanitizers), and hipcc into the gfx950 kernels (cutseq_amd/csrc/bam_kernels.hip.inc):
 * the field offsets, the record-fits test, every refusal in its order, the nibble table and the text length.  What
 * differs between the sides is how the bytes are moved (a loop here, 32 lanes per record on the device); nothing else.
 *
 * A record `rec[0 .. avail)` is the 4-byte block_size and the block behind it (all little-endian, at ANY byte address):
 *
 *    0 block_size i32     12 l_read_name u8    16 n_cigar_op u16    24 next_refID i32    36 read_name[l_read_name] (NUL-terminated)
 *    4 refID i32          13 mapq u8           18 flag u16          28 next_pos i32         cigar[4 * n_cigar_op]
 *    8 pos i32            14 bin u16           20 l_seq u32         32 tlen i32             seq[(l_seq + 1) / 2], qual[l_seq], tags
 *
 * and becomes  @<read_name without its NUL>\n<l_seq letters>\n+\n<qual[i] + 33>\n : 2 * l_seq + l_read_name + 5 bytes.
 *
 * Guarantees for any bytes whatsoever, given avail >= CSB_FIXED: csb_shape reads rec[0 .. 36) only; after CSB_OK from it,
 * name, cigar, seq and qual lie inside rec[0 .. avail), and csb_check reads nothing else; the expansion is called only
 * for a record csb_check passed.
 */
#ifndef CUTSEQ_BAM_H
#define CUTSEQ_BAM_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CSB_FN __host__ __device__ inline
#else
#define CSB_FN static inline
#endif

enum {
  CSB_OK = 0,
  /* the refusals, in the order they are tested: the first one that holds is the record's verdict.  The values are the
   * CS_TEXT_ERR_BAM_* codes of include/cutseq_hip.h */
  CSB_ERR_BLOCK_SIZE = 16,    /* block_size < 32, or the block leaves the bytes the record was given               */
  CSB_ERR_OVERRUN = 17,       /* fixed part + name + cigar + seq + qual exceed block_size                          */
  CSB_ERR_NAME = 18,          /* l_read_name == 0, or no NUL at read_name[l_read_name - 1]                          */
  CSB_ERR_ALIGNED = 19,       /* flag bit 0x4 is not set                                                           */
  CSB_ERR_NAME_LINE_END = 20, /* '\n' or '\r' inside the name                                                      */
  CSB_ERR_NO_QUAL = 21,       /* l_seq > 0 and qual[0] == 0xFF                                                     */
  CSB_ERR_QUAL_RANGE = 22     /* a quality above 93                                                                */
};

#define CSB_FIXED 36u      /* block_size and the fixed fields: the shortest record there is */
#define CSB_MIN_BLOCK 32u  /* ... as block_size counts it                                    */
#define CSB_FLAG_UNMAPPED 0x4u
#define CSB_MAX_QUAL 93u

CSB_FN uint32_t csb_u16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
CSB_FN uint32_t csb_u32(const uint8_t *p) {
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}

typedef struct csb_shape_t {
  uint32_t l_name; /* with its NUL */
  uint32_t l_seq;
  uint32_t flag;
  uint32_t name_at, seq_at, qual_at; /* offsets from the record's start */
  uint32_t text_len;                 /* bytes of the FASTQ record */
} csb_shape_t;

/* 2 * l_seq + l_read_name + 5; l_seq + (l_seq + 1) / 2 <= block_size < 2^31 keeps it below 2^32 */
CSB_FN uint32_t csb_text_len(uint32_t l_name, uint32_t l_seq) { return 2u * l_seq + l_name + 5u; }

/* The fixed fields of rec[0 .. avail), avail >= CSB_FIXED (and < 2^31): where the record's parts are, if they fit. */
CSB_FN int csb_shape(const uint8_t *rec, uint32_t avail, csb_shape_t *s) {
  const uint32_t block_size = csb_u32(rec);
  if (block_size < CSB_MIN_BLOCK || block_size >= 0x80000000u || block_size + 4u > avail) return CSB_ERR_BLOCK_SIZE;
  s->l_name = rec[12];
  const uint32_t n_cigar = csb_u16(rec + 16);
  s->flag = csb_u16(rec + 18);
  s->l_seq = csb_u32(rec + 20);
  const uint64_t need = (uint64_t)CSB_MIN_BLOCK + s->l_name + 4ull * n_cigar + ((uint64_t)s->l_seq + 1u) / 2u + s->l_seq;
  if (need > block_size) return CSB_ERR_OVERRUN;
  s->name_at = CSB_FIXED;
  s->seq_at = CSB_FIXED + s->l_name + 4u * n_cigar;
  s->qual_at = s->seq_at + (s->l_seq + 1u) / 2u;
  s->text_len = csb_text_len(s->l_name, s->l_seq);
  return CSB_OK;
}

/* the bytes of a dword that are above CSB_MAX_QUAL: bit 7 of each such byte (exact) */
CSB_FN uint32_t csb_qual_above(uint32_t v) {
  return (((v & 0x7f7f7f7fu) + (127u - CSB_MAX_QUAL) * 0x01010101u) | v) & 0x80808080u;
}

/* What is left to refuse once the shape stands (the device shares the quality scan over lanes if it likes; the verdict
 * is this one). */
CSB_FN int csb_check(const uint8_t *rec, const csb_shape_t *s) {
  if (s->l_name == 0u || rec[s->name_at + s->l_name - 1u] != 0u) return CSB_ERR_NAME;
  if (!(s->flag & CSB_FLAG_UNMAPPED)) return CSB_ERR_ALIGNED;
  for (uint32_t i = 0; i + 1u < s->l_name; ++i) {
    const uint8_t c = rec[s->name_at + i];
    if (c == '\n' || c == '\r') return CSB_ERR_NAME_LINE_END;
  }
  if (s->l_seq && rec[s->qual_at] == 0xFFu) return CSB_ERR_NO_QUAL;
  const uint8_t *q = rec + s->qual_at;
  uint32_t i = 0;
  for (; i + 4u <= s->l_seq; i += 4u)
    if (csb_qual_above(csb_u32(q + i))) return CSB_ERR_QUAL_RANGE;
  for (; i < s->l_seq; ++i)
    if (q[i] > CSB_MAX_QUAL) return CSB_ERR_QUAL_RANGE;
  return CSB_OK;
}

/* "=ACMGRSVTWYHKDBN" as two 64-bit words (a register pair each on the device): entry n is byte n & 7 of word n >> 3 */
#define CSB_LETTERS_LO 0x565352474d43413dull /* = A C M G R S V, '=' in the lowest byte */
#define CSB_LETTERS_HI 0x4e42444b48595754ull /* T W Y H K D B N */

CSB_FN uint32_t csb_letter(uint32_t nibble) {
  const uint64_t w = (nibble & 8u) ? CSB_LETTERS_HI : CSB_LETTERS_LO;
  return (uint32_t)(w >> ((nibble & 7u) * 8u)) & 0xffu;
}

/* four packed bytes (a little-endian dword, first byte lowest) -> their eight letters as two dwords, in text order */
CSB_FN void csb_letters8(uint32_t packed, uint32_t *lo, uint32_t *hi) {
  *lo = csb_letter((packed >> 4) & 15u) | csb_letter(packed & 15u) << 8 | csb_letter((packed >> 12) & 15u) << 16 |
        csb_letter((packed >> 8) & 15u) << 24;
  *hi = csb_letter((packed >> 20) & 15u) | csb_letter((packed >> 16) & 15u) << 8 | csb_letter(packed >> 28) << 16 |
        csb_letter((packed >> 24) & 15u) << 24;
}

/* The whole record, one byte after the other: the host form of the device's bam_expand.  Writes out[0 .. text_len). */
CSB_FN void csb_expand(const uint8_t *rec, const csb_shape_t *s, uint8_t *out) {
  uint32_t at = 0;
  out[at++] = '@';
  for (uint32_t i = 0; i + 1u < s->l_name; ++i) out[at++] = rec[s->name_at + i];
  out[at++] = '\n';
  uint32_t i = 0;
  for (; i + 8u <= s->l_seq; i += 8u) {
    uint32_t lo, hi;
    csb_letters8(csb_u32(rec + s->seq_at + i / 2u), &lo, &hi);
    for (uint32_t k = 0; k < 4u; ++k) out[at++] = (uint8_t)(lo >> (8u * k));
    for (uint32_t k = 0; k < 4u; ++k) out[at++] = (uint8_t)(hi >> (8u * k));
  }
  for (; i < s->l_seq; ++i) {
    const uint32_t byte = rec[s->seq_at + i / 2u];
    out[at++] = (uint8_t)csb_letter((i & 1u) ? byte & 15u : byte >> 4);
  }
  out[at++] = '\n';
  out[at++] = '+';
  out[at++] = '\n';
  for (i = 0; i < s->l_seq; ++i) out[at++] = (uint8_t)(rec[s->qual_at + i] + 33u);
  out[at++] = '\n';
}

#endif /* CUTSEQ_BAM_H */
