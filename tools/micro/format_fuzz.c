/* Sanitizer fuzz of the host formatter (csrc/cutseq_host.c, csh_format_chunk): small random chunks -- names of arbitrary
 * bytes, reads of length 0 and up, results inside their reads, random flags, xflags and bins, paired and single-end --
 * formatted without bins and with bins.  Every output buffer is a heap block of exactly the documented capacity (the
 * mate's raw text + 528 per record + 16), and the second binned run gets bin regions of exactly the bytes the first one's
 * size pass reported, so AddressSanitizer aborts on the first byte written past either.  Checked besides: out_len <=
 * capacity; every bin holds bin_off[b + 1] - bin_off[b] bytes (4 lines per counted record, none left over); the sizes of
 * the size pass (record_bytes) add up to the bytes the plain run's emit wrote for the same records.
 *   gcc -O1 -g -fsanitize=address,undefined -std=gnu11 -o /tmp/format_fuzz tools/micro/format_fuzz.c \
 *       cutseq_amd/csrc/cutseq_host.c cutseq_amd/csrc/pinflate.c -lpthread && /tmp/format_fuzz 5000
 * (5 000 iterations, a second: "fuzz done: 5000 chunks, 4862 formatted, 138 with differing ids", no report) */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the formatter's argument structs, as cutseq_host.c defines them (csh_format_struct_sizes tells a drift) */
typedef struct { uint16_t start, stop, cap_off; uint8_t cap_len, flags; } csh_result;
typedef struct { uint16_t off; uint8_t len, pad; } csh_cap2;
typedef struct {
  int32_t paired, has_umi, untrimmed_filter, reverse_complement;
  uint8_t flag_too_short, flag_untrimmed, pad[2];
  const char *suffix1[2], *suffix2[2];
} csh_format_params;
typedef struct { const uint8_t *raw; const int64_t *name_off; const int32_t *name_len; const uint8_t *seq, *qual; const csh_result *res; const uint8_t *xflags; } csh_mate;
typedef struct { int64_t n; uint32_t stride; csh_mate mate[2]; const csh_cap2 *cap2; const uint8_t *bin; int32_t n_bins; } csh_chunk;
typedef struct { uint8_t *out[3][2]; int64_t out_len[3][2], counts[3]; uint8_t *binned[2]; int64_t *bin_off, *bin_counts; } csh_format_out;
int64_t csh_format_chunk(const csh_format_params *, const csh_chunk *, csh_format_out *);
void csh_format_struct_sizes(int64_t sizes[3]);

static uint64_t rs = 88172645463325252ull;
static uint32_t rnd(void) { rs ^= rs << 13; rs ^= rs >> 7; rs ^= rs << 17; return (uint32_t)(rs >> 11); }
static uint8_t no_newline(void) { uint8_t c = (uint8_t)rnd(); return c == '\n' ? 'N' : c; }
static void *exact(size_t n) { void *p = malloc(n ? n : 1); if (!p) abort(); return p; }
#define FAIL(...) do { printf("it %d: ", it); printf(__VA_ARGS__); printf("\n"); return 1; } while (0)

enum { MAXN = 48, MAXLEN = 300, MAXNAME = 40 };

int main(int argc, char **argv) {
  const int iters = argc > 1 ? atoi(argv[1]) : 5000;
  int64_t sizes[3];
  csh_format_struct_sizes(sizes);
  if (sizes[0] != sizeof(csh_format_params) || sizes[1] != sizeof(csh_chunk) || sizes[2] != sizeof(csh_format_out)) {
    printf("struct definitions differ from cutseq_host.c\n");
    return 1;
  }
  static const char *const suffixes[] = {NULL, "/1", "/2", " x", ""};
  long formatted = 0, differing = 0;
  for (int it = 0; it < iters; ++it) {
    const int paired = rnd() & 1, mates = paired ? 2 : 1, n = rnd() % (MAXN + 1);
    const int n_bins = (rnd() & 3) == 0 ? 255 : 1 + rnd() % 6, longest = (rnd() & 1) ? 12 : MAXLEN;
    csh_format_params fp = {paired, rnd() & 1, rnd() & 1, rnd() & 1, 0x20, 0x40, {0, 0},
                            {suffixes[rnd() % 5], suffixes[rnd() % 5]}, {suffixes[rnd() % 5], suffixes[rnd() % 5]}};
    csh_chunk ck;
    memset(&ck, 0, sizeof ck);
    ck.n = n;
    ck.stride = 4;
    /* lengths and names first: the stride and the size of the raw text follow from them */
    int len[2][MAXN], nl[2][MAXN];
    uint8_t name[2][MAXN][MAXNAME];
    for (int i = 0; i < n; i++)
      for (int m = 0; m < mates; m++) {
        len[m][i] = (rnd() & 7) == 0 ? 0 : rnd() % (longest + 1);
        if ((uint32_t)(len[m][i] + 3) / 4 * 4 > ck.stride) ck.stride = (uint32_t)(len[m][i] + 3) / 4 * 4;
        if (m == 1 && rnd() % 512) { /* the mate's name: the same, or the same with another comment */
          nl[1][i] = nl[0][i];
          memcpy(name[1][i], name[0][i], MAXNAME);
          int sep = 0;
          while (sep < nl[1][i] && name[1][i][sep] != ' ' && name[1][i][sep] != '\t') sep++;
          for (int k = sep + 1; k < nl[1][i] && (rnd() & 1); k++) name[1][i][k] = no_newline();
          continue;
        }
        nl[m][i] = rnd() % (MAXNAME + 1);
        for (int k = 0; k < nl[m][i]; k++) name[m][i][k] = (rnd() & 3) == 0 ? " \t/12_\x1c"[rnd() % 7] : no_newline();
      }
    size_t cap[2] = {16, 16};
    void *owned[2][8];
    for (int m = 0; m < mates; m++) {
      size_t raw_len = 0;
      for (int i = 0; i < n; i++) raw_len += (size_t)nl[m][i] + 2 * (size_t)len[m][i] + 6;
      uint8_t *raw = exact(raw_len), *p = raw, *seq = exact((size_t)n * ck.stride), *qual = exact((size_t)n * ck.stride);
      int64_t *name_off = exact((size_t)n * 8);
      int32_t *name_len = exact((size_t)n * 4);
      csh_result *res = exact((size_t)n * sizeof *res);
      uint8_t *xf = (rnd() & 1) ? exact((size_t)n) : NULL;
      for (int i = 0; i < n; i++) {
        uint8_t *s = seq + (size_t)i * ck.stride, *q = qual + (size_t)i * ck.stride;
        const int L = len[m][i];
        for (int k = 0; k < L; k++) { s[k] = (rnd() & 1) ? "ACGTNacgtn"[rnd() % 10] : no_newline(); q[k] = no_newline(); }
        *p++ = '@'; name_off[i] = p - raw; name_len[i] = nl[m][i]; memcpy(p, name[m][i], (size_t)nl[m][i]); p += nl[m][i];
        *p++ = '\n'; memcpy(p, s, (size_t)L); p += L; *p++ = '\n'; *p++ = '+'; *p++ = '\n'; memcpy(p, q, (size_t)L); p += L; *p++ = '\n';
        res[i].stop = (uint16_t)(rnd() % (L + 1));
        res[i].start = (uint16_t)(rnd() % (res[i].stop + 1));
        res[i].cap_off = (uint16_t)(rnd() % (L + 1));
        res[i].cap_len = (uint8_t)(rnd() % ((L - res[i].cap_off > 255 ? 255 : L - res[i].cap_off) + 1));
        res[i].flags = (uint8_t)(rnd() & 0x9f) | ((rnd() & 7) == 0 ? 0x20 : 0) | ((rnd() & 3) == 0 ? 0x40 : 0);
        if (xf) xf[i] = (rnd() & 3) == 0 ? (uint8_t)(rnd() & 7) : 0;
      }
      ck.mate[m] = (csh_mate){raw, name_off, name_len, seq, qual, res, xf};
      cap[m] = raw_len + 528 * (size_t)n + 16;
      void *all[8] = {raw, seq, qual, name_off, name_len, res, xf, NULL};
      memcpy(owned[m], all, sizeof all);
    }
    csh_cap2 *cap2 = (!paired && (rnd() & 1)) ? exact((size_t)n * sizeof *cap2) : NULL;
    uint8_t *bin = exact((size_t)n);
    for (int i = 0; i < n; i++) {
      bin[i] = (rnd() & 7) == 0 ? 0xff : (uint8_t)(rnd() % (n_bins + 1)); /* n_bins itself: out of range */
      if (cap2) { cap2[i].off = (uint16_t)(rnd() % (len[0][i] + 1)); cap2[i].len = (uint8_t)(rnd() % ((len[0][i] - cap2[i].off > 255 ? 255 : len[0][i] - cap2[i].off) + 1)); cap2[i].pad = 0; }
    }
    ck.cap2 = cap2;

    /* runs: 0 without bins; 1 with bins, the bin regions at the documented capacity; 2 with bins, the regions at exactly
     * the bytes run 1 reported */
    csh_format_out o[3];
    int64_t bin_off[3][2 * 256], bin_counts[3][255];
    int failed = 0;
    memset(o, 0, sizeof o);
    for (int run = 0; run < 3 && !failed; run++) {
      for (int r = 0; r < 3; r++) for (int m = 0; m < 2; m++) o[run].out[r][m] = exact(cap[m]);
      ck.n_bins = run ? n_bins : 0;
      ck.bin = run ? bin : NULL;
      for (int m = 0; m < 2 && run; m++) {
        size_t want = run == 1 ? cap[m] : (size_t)bin_off[1][m * (n_bins + 1) + n_bins];
        o[run].binned[m] = exact(want);
        memset(o[run].binned[m], 0, want ? want : 1);
      }
      o[run].bin_off = run ? bin_off[run] : NULL;
      o[run].bin_counts = run ? bin_counts[run] : NULL;
      int64_t rc = csh_format_chunk(&fp, &ck, &o[run]);
      if (rc < -(int64_t)n || rc > 0 || (rc < 0 && !paired)) FAIL("run %d returned %lld", run, (long long)rc);
      if (rc < 0) failed = 1;
    }
    if (failed) differing++; else formatted++;
    for (int m = 0; m < mates && !failed; m++) {
      const int64_t *off1 = bin_off[1] + m * (n_bins + 1), *off2 = bin_off[2] + m * (n_bins + 1);
      for (int run = 0; run < 3; run++)
        for (int r = 0; r < 3; r++)
          if (o[run].out_len[r][m] < 0 || (size_t)o[run].out_len[r][m] > cap[m]) FAIL("out_len beyond the capacity");
      if (off1[0] != 0 || memcmp(off1, off2, (size_t)(n_bins + 1) * 8) || memcmp(bin_counts[1], bin_counts[2], (size_t)n_bins * 8))
        FAIL("the two binned runs disagree");
      if ((size_t)off1[n_bins] > cap[m]) FAIL("bins beyond the capacity");
      for (int b = 0; b < n_bins; b++) { /* the bin is full of whole records: 4 lines each, the last byte a newline */
        int64_t lines = 0;
        for (int64_t k = off2[b]; k < off2[b + 1]; k++) lines += o[2].binned[m][k] == '\n';
        if (lines != 4 * bin_counts[2][b] || (off2[b + 1] > off2[b] && o[2].binned[m][off2[b + 1] - 1] != '\n')) FAIL("bin %d of mate %d is not filled exactly", b, m);
        if (memcmp(o[1].binned[m] + off1[b], o[2].binned[m] + off2[b], (size_t)(off2[b + 1] - off2[b]))) FAIL("bin bytes differ between runs");
      }
      /* the trimmed records without a barcode go to route 2, the others into the bins: record_bytes summed == emit's bytes */
      if (o[0].out_len[0][m] + o[0].out_len[2][m] != off2[n_bins] + o[2].out_len[2][m]) FAIL("record_bytes and emit disagree");
      if (o[2].out_len[0][m] != 0 || o[0].out_len[1][m] != o[2].out_len[1][m] ||
          memcmp(o[0].out[1][m], o[2].out[1][m], (size_t)o[0].out_len[1][m])) FAIL("routes differ between the plain and the binned run");
    }
    if (!failed) {
      int64_t in_bins = 0;
      for (int b = 0; b < n_bins; b++) in_bins += bin_counts[2][b];
      if (o[2].counts[0] != 0 || o[0].counts[1] != o[2].counts[1] || o[0].counts[0] + o[0].counts[2] != in_bins + o[2].counts[2])
        FAIL("counts differ between the plain and the binned run");
    }
    for (int run = 0; run < 3; run++) {
      for (int r = 0; r < 3; r++) for (int m = 0; m < 2; m++) free(o[run].out[r][m]);
      free(o[run].binned[0]);
      free(o[run].binned[1]);
    }
    for (int m = 0; m < mates; m++) for (int k = 0; k < 7; k++) free(owned[m][k]);
    free(cap2);
    free(bin);
  }
  printf("fuzz done: %d chunks, %ld formatted, %ld with differing ids\n", iters, formatted, differing);
  return 0;
}
