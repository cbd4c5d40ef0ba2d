/*
 * cutseq_inflate.h -- RFC 1951 decoder of ONE BGZF block's deflate payload, host and device form.
 *
 * Every decision that keeps the decoder inside its buffers lives here as plain C++ that g++ compiles for the host
 * (tools/inflate_host_check.cpp runs it under the sanitizers, "one lane") and hipcc for gfx950
 * (cutseq_amd/csrc/inflate_kernels.hip.inc, one wavefront per block): the bit reader, header parsing, table
 * construction, symbol decode and the bounds checks.  What differs between the two is how the bytes are moved (the
 * `Sink` template parameter) and how the lanes' CRC slices are combined; nothing else.
 *
 * Lanes.  Every function takes `lane` / `nl` (host: 0 / 1; device: the lane id / 64).  All lanes run the symbol loop on
 * the same values -- bit buffer, symbols and every branch are uniform across the lanes -- and share one csi_shared
 * (LDS on the device).  Loops that fill tables are strided by `nl`; CSI_SYNC() separates a table's writers from
 * its readers (nothing on the host).
 *
 * Guarantees for any input bytes whatsoever:
 *   - reads only comp[0 .. comp_len): the bit reader hands out bits it has, a request past the end is CSI_ERR_INPUT;
 *   - writes only out[0 .. out_len): a literal or a match that does not fit is CSI_ERR_OUTPUT, checked before the Sink
 *     is called;
 *   - a distance never reaches in front of out[0] (CSI_ERR_DISTANCE);
 *   - termination: every loop turn consumes at least one input bit or ends with an error, and the symbol loop of a
 *     deflate block carries a budget of (room left in out) + 1 turns.
 * Codes are accepted and refused as zlib does (inflate_table): over-subscribed sets never, incomplete sets only for
 * the literal/length and distance codes when no code is longer than one bit.
 */
#ifndef CUTSEQ_INFLATE_H
#define CUTSEQ_INFLATE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CSI_FN __host__ __device__ inline
#else
#define CSI_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define CSI_SYNC() __syncthreads()
#define CSI_UNIFORM(x) ((uint32_t)__builtin_amdgcn_readfirstlane((int)(x)))
#else
#define CSI_SYNC() ((void)0)
#define CSI_UNIFORM(x) ((uint32_t)(x))
#endif

enum {
  CSI_OK = 0,
  CSI_ERR_BTYPE = 1,     /* block type 3                                                             */
  CSI_ERR_STORED = 2,    /* stored block: LEN != ~NLEN                                               */
  CSI_ERR_CODE = 3,      /* over-subscribed code, incomplete code zlib refuses, HLIT > 286, HDIST > 30 */
  CSI_ERR_REPEAT = 4,    /* code-length repeat without a predecessor, or running past HLIT + HDIST   */
  CSI_ERR_NO_EOB = 5,    /* the literal/length code has no end-of-block symbol                       */
  CSI_ERR_SYMBOL = 6,    /* a bit pattern that is no code, length symbol 286/287, distance symbol 30/31 */
  CSI_ERR_INPUT = 7,     /* the payload ends inside the stream                                       */
  CSI_ERR_OUTPUT = 8,    /* more text than out_len                                                   */
  CSI_ERR_DISTANCE = 9,  /* a match reaches in front of the block's own text                         */
  CSI_ERR_ISIZE = 10,    /* the stream ended with less text than out_len (ISIZE)                     */
  CSI_ERR_CRC = 11,      /* CRC-32 of the text differs from the trailer's                            */
  CSI_ERR_TRAILING = 12  /* whole payload bytes behind the final block (zlib: unused input)          */
};

#define CSI_FAST 10        /* bits of the one-step table; longer codes take the canonical walk */
#define CSI_MAX_LENS 320   /* 288 + 32 */
#define CSI_CRC_POLY 0xedb88320u

struct csi_bits {
  const uint8_t *p; /* the payload: p[0 .. end) and not a byte more */
  uint32_t pos, end;
  uint64_t buf;     /* bits [0, n) are the next n bits of the stream; bits above n are stream bits too, or zero */
  uint32_t n;
  uint32_t err;
};

struct csi_huff {
  uint16_t fast[1 << CSI_FAST]; /* symbol << 4 | code length, 0: not a code of <= CSI_FAST bits */
  uint16_t count[16];           /* codes per length */
  uint16_t first[16];           /* canonical code of the first symbol of each length */
  uint16_t base[16];            /* its index in sym */
  uint16_t sym[288];            /* symbols by (length, value) */
};

struct csi_shared {
  csi_huff lit, dist; /* (the code-length code lives in `dist` until the distance code is built) */
  uint8_t lens[CSI_MAX_LENS];
  uint32_t crc_tab[256];
};

/* ---- bit reader ----------------------------------------------------------------------------------------------- */

CSI_FN void csi_bits_init(csi_bits &b, const uint8_t *p, uint32_t len) {
  b.p = p;
  b.pos = 0;
  b.end = len;
  b.buf = 0;
  b.n = 0;
  b.err = CSI_OK;
}

/* At least 56 bits in the buffer unless the payload has fewer left. */
CSI_FN void csi_refill(csi_bits &b) {
  if ((uint64_t)b.pos + 8 <= b.end) {
    uint64_t w;
    __builtin_memcpy(&w, b.p + b.pos, 8);
    b.buf |= w << b.n;
    const uint32_t adv = (63 - b.n) >> 3;
    b.pos += adv;
    b.n += adv * 8;
  } else {
    while (b.n <= 56 && b.pos < b.end) {
      b.buf |= (uint64_t)b.p[b.pos++] << b.n;
      b.n += 8;
    }
  }
}

/* k <= 16 bits; past the end: CSI_ERR_INPUT and 0 */
CSI_FN uint32_t csi_take(csi_bits &b, uint32_t k) {
  if (b.n < k) {
    b.err = CSI_ERR_INPUT;
    return 0;
  }
  const uint32_t v = (uint32_t)b.buf & ((1u << k) - 1u);
  b.buf >>= k;
  b.n -= k;
  return v;
}

/* ---- tables ------------------------------------------------------------------------------------------------- */

enum { CSI_KIND_CODES = 0, CSI_KIND_LENS = 1, CSI_KIND_DISTS = 2 };

CSI_FN uint32_t csi_bitrev(uint32_t code, uint32_t len) {
  uint32_t r = 0;
  for (uint32_t i = 0; i < len; ++i) r |= ((code >> i) & 1u) << (len - 1 - i);
  return r;
}

/* The decoding table of the canonical code with lengths lens[0 .. n), n <= 288.  CSI_OK or CSI_ERR_CODE. */
CSI_FN uint32_t csi_build(csi_huff &h, const uint8_t *lens, uint32_t n, int kind, uint32_t lane, uint32_t nl) {
  for (uint32_t l = lane; l < 16; l += nl) {
    uint32_t c = 0;
    for (uint32_t i = 0; i < n; ++i) c += lens[i] == l;
    h.count[l] = (uint16_t)c;
  }
  for (uint32_t i = lane; i < (1u << CSI_FAST); i += nl) h.fast[i] = 0;
  CSI_SYNC();
  int left = 1;
  uint32_t code = 0, idx = 0, longest = 0;
  bool over = false;
  for (uint32_t l = 1; l < 16; ++l) {
    const uint32_t c = h.count[l];
    left = (left << 1) - (int)c;
    if (left < 0) {
      over = true;
      left = 0; /* (keeps the shifts defined; the verdict is fixed) */
    }
    if (c) longest = l;
    if (lane == 0) {
      h.first[l] = (uint16_t)code;
      h.base[l] = (uint16_t)idx;
    }
    code = (code + c) << 1;
    idx += c;
  }
  CSI_SYNC();
  if (over) return CSI_ERR_CODE;
  if (left > 0 && (kind == CSI_KIND_CODES || longest > 1)) return CSI_ERR_CODE;
  for (uint32_t l = 1 + lane; l < 16; l += nl) {
    uint32_t k = h.base[l];
    for (uint32_t i = 0; i < n; ++i)
      if (lens[i] == l) h.sym[k++] = (uint16_t)i; /* k < base[l] + count[l] <= idx <= n <= 288 */
  }
  CSI_SYNC();
  for (uint32_t j = lane; j < idx; j += nl) {
    const uint32_t s = h.sym[j], l = lens[s];
    if (l <= CSI_FAST) {
      const uint32_t r = csi_bitrev(h.first[l] + (j - h.base[l]), l);
      for (uint32_t k = r; k < (1u << CSI_FAST); k += 1u << l) h.fast[k] = (uint16_t)(s << 4 | l);
    }
  }
  CSI_SYNC();
  return CSI_OK;
}

/* The next symbol, or -1 with b.err set (CSI_ERR_SYMBOL: no such code; CSI_ERR_INPUT: the payload ended in it). */
CSI_FN int csi_decode(const csi_huff &h, csi_bits &b) {
  const uint32_t e = h.fast[(uint32_t)b.buf & ((1u << CSI_FAST) - 1u)];
  uint32_t l = e & 15u;
  int sym = (int)(e >> 4);
  if (l == 0) {
    int code = 0, first = 0, index = 0;
    sym = -1;
    for (l = 1; l < 16; ++l) {
      code |= (int)((b.buf >> (l - 1)) & 1u);
      const int c = h.count[l];
      if (code - c < first) {
        sym = h.sym[index + (code - first)]; /* index + code - first < index + c <= 288 */
        break;
      }
      index += c;
      first = (first + c) << 1;
      code <<= 1;
    }
    if (sym < 0) {
      b.err = CSI_ERR_SYMBOL;
      return -1;
    }
  }
  if (b.n < l) {
    b.err = CSI_ERR_INPUT;
    return -1;
  }
  b.buf >>= l;
  b.n -= l;
  return (int)CSI_UNIFORM(sym);
}

/* ---- CRC-32 ------------------------------------------------------------------------------------------------- */

CSI_FN void csi_crc_table(uint32_t *tab, uint32_t lane, uint32_t nl) {
  for (uint32_t i = lane; i < 256; i += nl) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ CSI_CRC_POLY : c >> 1;
    tab[i] = c;
  }
}

/* a * b modulo the CRC polynomial, reflected bit order (bit 31 is x^0) */
CSI_FN uint32_t csi_mulmod(uint32_t a, uint32_t b) {
  uint32_t p = 0;
  for (uint32_t m = 1u << 31; m; m >>= 1) {
    if (a & m) p ^= b;
    b = (b & 1u) ? (b >> 1) ^ CSI_CRC_POLY : b >> 1;
  }
  return p;
}

/* x^(8 * nbytes) */
CSI_FN uint32_t csi_xpow8(uint64_t nbytes) {
  uint32_t r = 1u << 31, s = 1u << 23; /* x^0, x^8 */
  for (; nbytes; nbytes >>= 1) {
    if (nbytes & 1u) r = csi_mulmod(s, r);
    s = csi_mulmod(s, s);
  }
  return r;
}

/* The text of n bytes sits right-aligned in a frame of `nl` slices of S = ceil(n / nl) bytes: zeros in front do not
 * change a CRC register that starts at zero.  -> the raw (zero init, no final xor) CRC of slice `lane`, and the '\n'
 * in it. */
CSI_FN uint32_t csi_crc_slice(const uint8_t *text, uint32_t n, const uint32_t *tab, uint32_t lane, uint32_t nl,
                              uint32_t *newlines) {
  const uint32_t S = (n + nl - 1) / nl, pad = S * nl - n;
  const uint32_t lo = lane * S, hi = lo + S; /* frame offsets */
  uint32_t crc = 0, lines = 0;
  for (uint32_t f = lo < pad ? pad : lo; f < hi; ++f) {
    const uint32_t c = text[f - pad]; /* f - pad < S * nl - pad = n */
    lines += c == '\n';
    crc = tab[(crc ^ c) & 0xffu] ^ (crc >> 8);
  }
  *newlines = lines;
  return crc;
}

/* raw CRC of A || B from the raw CRCs of A and B, `shift` = x^(8 |B|) */
CSI_FN uint32_t csi_crc_join(uint32_t crc_a, uint32_t crc_b, uint32_t shift) { return csi_mulmod(shift, crc_a) ^ crc_b; }

/* the CRC-32 of gzip from the raw CRC of the whole text of n bytes: init and final xor, moved behind the data */
CSI_FN uint32_t csi_crc_final(uint32_t raw, uint32_t n) { return raw ^ csi_mulmod(csi_xpow8(n), 0xffffffffu) ^ 0xffffffffu; }

/* ---- the stream --------------------------------------------------------------------------------------------- */

/* Sink: how bytes reach out[].  The decoder has checked every position before it calls:
 *   lit(pos, byte)            out[pos] = byte                       pos < out_len
 *   match(pos, len, dist)     out[pos + i] = out[pos + i - dist]    1 <= dist <= pos, pos + len <= out_len
 *   stored(pos, src, len)     out[pos + i] = src[i]                 src[0 .. len) inside the payload, pos + len <= out_len
 *   finish(pos)               everything written so far is visible to every lane */
struct csi_host_sink {
  uint8_t *out;
  void lit(uint32_t pos, uint32_t byte) { out[pos] = (uint8_t)byte; }
  void match(uint32_t pos, uint32_t len, uint32_t dist) {
    for (uint32_t i = 0; i < len; ++i) out[pos + i] = out[pos + i - dist];
  }
  void stored(uint32_t pos, const uint8_t *src, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) out[pos + i] = src[i];
  }
  void finish(uint32_t) {}
};

CSI_FN uint32_t csi_fixed_tables(csi_shared &sh, uint32_t lane, uint32_t nl) {
  for (uint32_t i = lane; i < 288; i += nl) sh.lens[i] = (uint8_t)(i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8);
  for (uint32_t i = 288 + lane; i < 320; i += nl) sh.lens[i] = 5;
  CSI_SYNC();
  uint32_t rc = csi_build(sh.lit, sh.lens, 288, CSI_KIND_LENS, lane, nl);
  if (rc == CSI_OK) rc = csi_build(sh.dist, sh.lens + 288, 32, CSI_KIND_DISTS, lane, nl);
  return rc;
}

/* The header of a dynamic block -> both tables. */
CSI_FN uint32_t csi_dynamic_tables(csi_shared &sh, csi_bits &b, uint32_t lane, uint32_t nl) {
  csi_refill(b);
  const uint32_t hlit = csi_take(b, 5) + 257, hdist = csi_take(b, 5) + 1, hclen = csi_take(b, 4) + 4;
  if (b.err) return b.err;
  if (hlit > 286 || hdist > 30) return CSI_ERR_CODE;
  /* (all lanes store the same values below: each lane reads back what it wrote itself) */
  for (uint32_t i = 0; i < 19; ++i) sh.lens[i] = 0;
  for (uint32_t i = 0; i < hclen; ++i) {
    /* 16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15 */
    const uint32_t where = i < 3 ? 16 + i : i == 3 ? 0 : (i & 1u) ? 10 - ((i + 1) >> 1) : 6 + (i >> 1);
    csi_refill(b);
    sh.lens[where] = (uint8_t)csi_take(b, 3);
  }
  if (b.err) return b.err;
  CSI_SYNC();
  uint32_t rc = csi_build(sh.dist, sh.lens, 19, CSI_KIND_CODES, lane, nl);
  if (rc != CSI_OK) return rc;
  const uint32_t total = hlit + hdist; /* <= 316 < CSI_MAX_LENS */
  uint32_t idx = 0, prev = 0;
  while (idx < total) { /* every turn takes at least one bit or leaves */
    csi_refill(b);
    const int sym = csi_decode(sh.dist, b);
    if (sym < 0) return b.err;
    uint32_t rep = 1, val = (uint32_t)sym;
    if (sym == 16) {
      if (idx == 0) return CSI_ERR_REPEAT;
      val = prev;
      rep = 3 + csi_take(b, 2);
    } else if (sym == 17) {
      val = 0;
      rep = 3 + csi_take(b, 3);
    } else if (sym == 18) {
      val = 0;
      rep = 11 + csi_take(b, 7);
    } else if (sym > 18) {
      return CSI_ERR_SYMBOL;
    }
    if (b.err) return b.err;
    if (rep > total - idx) return CSI_ERR_REPEAT;
    for (uint32_t k = 0; k < rep; ++k) sh.lens[idx + k] = (uint8_t)val;
    idx += rep;
    prev = val;
  }
  if (sh.lens[256] == 0) return CSI_ERR_NO_EOB;
  CSI_SYNC();
  rc = csi_build(sh.lit, sh.lens, hlit, CSI_KIND_LENS, lane, nl);
  if (rc == CSI_OK) rc = csi_build(sh.dist, sh.lens + hlit, hdist, CSI_KIND_DISTS, lane, nl);
  return rc;
}

/* The deflate stream in comp[0 .. comp_len) -> out[0 .. out_len) through `o`.  -> CSI_OK when the stream's final block
 * ended and exactly out_len bytes were produced (CRC not looked at), else the verdict.  *produced: bytes written. */
template <class Sink>
CSI_FN uint32_t csi_inflate_stream(csi_shared &sh, const uint8_t *comp, uint32_t comp_len, uint32_t out_len, Sink &o,
                                   uint32_t lane, uint32_t nl, uint32_t *produced) {
  csi_bits b;
  csi_bits_init(b, comp, comp_len);
  uint32_t pos = 0, err = CSI_OK;
  bool final = false, have_fixed = false;
  while (!final && err == CSI_OK) { /* every turn takes at least the three header bits or leaves */
    csi_refill(b);
    final = CSI_UNIFORM(csi_take(b, 1)) != 0;
    const uint32_t type = CSI_UNIFORM(csi_take(b, 2));
    if (b.err) {
      err = b.err;
      break;
    }
    if (type == 3) {
      err = CSI_ERR_BTYPE;
      break;
    }
    if (type == 0) {
      csi_take(b, b.n & 7u); /* to the byte boundary: pos * 8 - n is the stream's bit position */
      csi_refill(b);
      const uint32_t len = CSI_UNIFORM(csi_take(b, 16)), nlen = CSI_UNIFORM(csi_take(b, 16));
      if (b.err) {
        err = b.err;
        break;
      }
      if (len != (nlen ^ 0xffffu)) {
        err = CSI_ERR_STORED;
        break;
      }
      b.pos -= b.n >> 3; /* whole bytes go back: the copy reads the payload itself */
      b.buf = 0;
      b.n = 0;
      if (len > b.end - b.pos) {
        err = CSI_ERR_INPUT;
        break;
      }
      if (len > out_len - pos) {
        err = CSI_ERR_OUTPUT;
        break;
      }
      o.stored(pos, b.p + b.pos, len);
      b.pos += len;
      pos += len;
      continue;
    }
    if (type == 1) {
      if (!have_fixed) err = csi_fixed_tables(sh, lane, nl);
      have_fixed = true;
    } else {
      err = csi_dynamic_tables(sh, b, lane, nl);
      have_fixed = false;
    }
    if (err != CSI_OK) break;
    uint32_t budget = out_len - pos + 1; /* symbols this block can hold: one per byte of room, and its end-of-block */
    for (;;) {
      if (budget-- == 0) {
        err = CSI_ERR_OUTPUT;
        break;
      }
      csi_refill(b); /* 56 bits: a length code, its extra bits, a distance code and its extra bits are 48 at most */
      int sym = csi_decode(sh.lit, b);
      if (sym < 0) {
        err = b.err;
        break;
      }
      if (sym < 256) {
        if (pos >= out_len) {
          err = CSI_ERR_OUTPUT;
          break;
        }
        o.lit(pos++, (uint32_t)sym);
        continue;
      }
      if (sym == 256) break;
      sym -= 257;
      if (sym >= 29) {
        err = CSI_ERR_SYMBOL;
        break;
      }
      uint32_t len, ext;
      if (sym < 8) {
        len = 3 + (uint32_t)sym;
        ext = 0;
      } else if (sym == 28) {
        len = 258;
        ext = 0;
      } else {
        ext = ((uint32_t)sym - 4) >> 2;
        len = ((4 + ((uint32_t)sym & 3u)) << ext) + 3;
      }
      len += csi_take(b, ext);
      const int ds = csi_decode(sh.dist, b);
      if (ds < 0) {
        err = b.err;
        break;
      }
      if (ds >= 30) {
        err = CSI_ERR_SYMBOL;
        break;
      }
      uint32_t dist;
      if (ds < 4) {
        dist = 1 + (uint32_t)ds;
      } else {
        const uint32_t dext = ((uint32_t)ds >> 1) - 1;
        dist = ((2 + ((uint32_t)ds & 1u)) << dext) + 1 + csi_take(b, dext);
      }
      if (b.err) {
        err = b.err;
        break;
      }
      len = CSI_UNIFORM(len);
      dist = CSI_UNIFORM(dist);
      if (dist > pos) {
        err = CSI_ERR_DISTANCE;
        break;
      }
      if (len > out_len - pos) {
        err = CSI_ERR_OUTPUT;
        break;
      }
      o.match(pos, len, dist);
      pos += len;
    }
  }
  o.finish(pos);
  *produced = pos;
  if (err == CSI_OK && pos != out_len) err = CSI_ERR_ISIZE;
  if (err == CSI_OK && (b.end - b.pos) + (b.n >> 3) != 0) err = CSI_ERR_TRAILING;
  return err;
}

#if !defined(__HIP_DEVICE_COMPILE__) || !__HIP_DEVICE_COMPILE__
/* Host form, "one lane": decode, then the CRC the way the device forms it -- `crc_lanes` slices of the right-aligned
 * frame, joined by log steps (crc_lanes a power of two; 64 restates the kernel, 1 is a plain table CRC). */
static inline uint32_t csi_inflate_block_host(const uint8_t *comp, uint32_t comp_len, uint8_t *out, uint32_t out_len,
                                              uint32_t want_crc, uint32_t crc_lanes, uint32_t *newlines) {
  static csi_shared sh; /* (7 KB; the check tool is single-threaded) */
  csi_host_sink sink{out};
  uint32_t produced = 0;
  *newlines = 0;
  uint32_t err = csi_inflate_stream(sh, comp, comp_len, out_len, sink, 0u, 1u, &produced);
  if (err != CSI_OK) return err;
  csi_crc_table(sh.crc_tab, 0, 1);
  uint32_t part[64], lines = 0;
  if (crc_lanes > 64) crc_lanes = 64;
  for (uint32_t l = 0; l < crc_lanes; ++l) {
    uint32_t got = 0;
    part[l] = csi_crc_slice(out, out_len, sh.crc_tab, l, crc_lanes, &got);
    lines += got;
  }
  const uint32_t S = (out_len + crc_lanes - 1) / crc_lanes;
  uint32_t shift = csi_xpow8(S);
  for (uint32_t step = 1; step < crc_lanes; step <<= 1) {
    for (uint32_t l = 0; l + step < crc_lanes; l += 2 * step) part[l] = csi_crc_join(part[l], part[l + step], shift);
    shift = csi_mulmod(shift, shift);
  }
  *newlines = lines;
  return csi_crc_final(part[0], out_len) == want_crc ? CSI_OK : CSI_ERR_CRC;
}
#endif

#endif /* CUTSEQ_INFLATE_H */
