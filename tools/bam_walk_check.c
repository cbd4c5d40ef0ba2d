// bam_walk_check -- the host walker and the shared record decisions of include/cutseq_bam.h as a program of its own.
//
//   gcc -O1 -g -std=gnu11 -fsanitize=address,undefined -fno-sanitize-recover=all -o bam_walk_check tools/bam_walk_check.c -lpthread
//   bam_walk_check cases.bin
//
// Reads a case file (tests/bam_rule.py: write_case_file): per case an inflated BAM stream and what the rule says about
// it -- the FASTQ text, or the first refusal in record order.  Every stream, every record and every record's text is a
// heap block of its exact size, so the sanitizer sees a byte read or written too far: csh_bam_header and csh_bam_walk run
// over the stream, then csb_shape, csb_check and csb_expand -- the decisions the kernels of bam_kernels.hip.inc compile
// -- over a copy of each record the walk found.  Prints the cases that differ and exits 1 if there are any.
#include <stdio.h>

#include "../cutseq_amd/csrc/cutseq_host.c" /* the walker (and cutseq_bam.h with it) */

enum { V_OK = 0, V_MAGIC = 1, V_HEADER_LENGTH = 2, V_ENDS_IN_HEADER = 3, V_ENDS_IN_RECORD = 4 };

static void *exact(size_t n) {
  void *p = malloc(n ? n : 1);
  if (!p) {
    fprintf(stderr, "out of memory\n");
    exit(70);
  }
  return p;
}

int main(int argc, char **argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
    return 64;
  }
  FILE *fh = fopen(argv[1], "rb");
  if (!fh) {
    perror(argv[1]);
    return 66;
  }
  char magic[4];
  uint32_t count = 0, differ = 0;
  if (fread(magic, 1, 4, fh) != 4 || memcmp(magic, "CSBC", 4) != 0 || fread(&count, 4, 1, fh) != 1) {
    fprintf(stderr, "%s: not a case file\n", argv[1]);
    return 65;
  }
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t head[4];
    if (fread(head, 4, 4, fh) != 4) {
      fprintf(stderr, "%s: truncated at case %u\n", argv[1], i);
      return 65;
    }
    const uint32_t n = head[0], want_code = head[1], want_record = head[2], want_len = head[3];
    uint8_t *stream = exact(n), *want = exact(want_len);
    if ((n && fread(stream, 1, n, fh) != n) || (want_len && fread(want, 1, want_len, fh) != want_len)) {
      fprintf(stderr, "%s: truncated in case %u\n", argv[1], i);
      return 65;
    }
    uint32_t code = V_OK, record = 0;
    uint8_t *text = NULL;
    uint64_t text_len = 0;
    const int64_t header = csh_bam_header(stream, n);
    if (header <= 0) {
      code = header == -1 ? V_MAGIC : (header == -2 ? V_HEADER_LENGTH : V_ENDS_IN_HEADER);
    } else {
      const int64_t room = n / CSB_FIXED + 1;
      uint32_t *offsets = exact((size_t)room * 4);
      int64_t next = 0, walk_text = 0;
      int32_t bad = 0;
      const int64_t found = csh_bam_walk(stream, n, header, room, offsets, &next, &walk_text, &bad);
      text = exact((size_t)walk_text);
      uint64_t fits = 0;
      for (int64_t r = 0; r < found; ++r) {
        const uint32_t at = offsets[r], end = r + 1 < found ? offsets[r + 1] : (uint32_t)next;
        uint8_t *rec = exact(end - at);
        memcpy(rec, stream + at, end - at);
        csb_shape_t s;
        int verdict = csb_shape(rec, end - at, &s);
        if (verdict == CSB_OK) {
          fits += s.text_len;
          verdict = csb_check(rec, &s);
        }
        if (verdict == CSB_OK && code == V_OK) {
          uint8_t *one = exact(s.text_len);
          csb_expand(rec, &s, one);
          memcpy(text + text_len, one, s.text_len);
          text_len += s.text_len;
          free(one);
        } else if (code == V_OK) {
          code = (uint32_t)verdict;
          record = (uint32_t)r;
        }
        free(rec);
      }
      if (fits != (uint64_t)walk_text) {
        printf("case %u: the walk sizes the text at %lld bytes, its records give %llu\n", i, (long long)walk_text,
               (unsigned long long)fits);
        ++differ;
      }
      if (code == V_OK && bad) {
        code = CSB_ERR_BLOCK_SIZE;
        record = (uint32_t)found;
      } else if (code == V_OK && next < (int64_t)n) {
        code = V_ENDS_IN_RECORD;
        record = (uint32_t)found;
      }
      free(offsets);
    }
    const int same_text = code != V_OK || (text_len == want_len && (want_len == 0 || memcmp(text, want, want_len) == 0));
    if (code != want_code || (code != V_OK && code >= V_ENDS_IN_RECORD && record != want_record) || !same_text) {
      printf("case %u: verdict %u at record %u (%llu bytes of text), the rule says %u at record %u (%u bytes)\n", i, code, record,
             (unsigned long long)text_len, want_code, want_record, want_len);
      ++differ;
    }
    free(text);
    free(stream);
    free(want);
  }
  fclose(fh);
  printf("%u cases, %u differ\n", count, differ);
  return differ ? 1 : 0;
}
