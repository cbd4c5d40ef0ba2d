// inflate_host_check -- the shared decoder of include/cutseq_inflate.h, "one lane", as a program of its own.
//
//   g++ -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -o inflate_host_check tools/inflate_host_check.cpp
//   inflate_host_check cases.bin
//
// Reads a case file (tests/bgzf_rule.py: write_case_file) and prints one line per case:
//   <index> <verdict> <adler32 of the text, 0 when refused> <newlines> <guards: 1 untouched, 0 written>
// Every payload and every output region is a heap block of its exact size (the sanitizer sees a byte too far on either
// side); the output region sits between guard bytes inside its block, which catches writes the decoder thinks legal.
// The CRC is formed twice, as one slice and as the device's 64 slices joined by log steps; a difference is exit 2.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "cutseq_inflate.h"

static const uint32_t kGuard = 64;

static uint32_t adler32(const uint8_t *p, uint32_t n) {
  uint32_t a = 1, b = 0;
  for (uint32_t i = 0; i < n; ++i) {
    a = (a + p[i]) % 65521u;
    b = (b + a) % 65521u;
  }
  return b << 16 | a;
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
  uint32_t count = 0;
  if (fread(magic, 1, 4, fh) != 4 || memcmp(magic, "CSIC", 4) != 0 || fread(&count, 4, 1, fh) != 1) {
    fprintf(stderr, "%s: not a case file\n", argv[1]);
    return 65;
  }
  for (uint32_t i = 0; i < count; ++i) {
    uint32_t head[3];
    if (fread(head, 4, 3, fh) != 3) {
      fprintf(stderr, "%s: truncated at case %u\n", argv[1], i);
      return 65;
    }
    const uint32_t comp_len = head[0], out_len = head[1], crc = head[2];
    uint8_t *comp = (uint8_t *)malloc(comp_len ? comp_len : 1);
    if (comp_len && fread(comp, 1, comp_len, fh) != comp_len) {
      fprintf(stderr, "%s: truncated in case %u\n", argv[1], i);
      return 65;
    }
    uint8_t *frame = (uint8_t *)malloc((size_t)out_len + 2 * kGuard);
    memset(frame, 0xA5, (size_t)out_len + 2 * kGuard);
    uint8_t *out = frame + kGuard;
    uint32_t lines = 0, lines1 = 0;
    const uint32_t verdict = csi_inflate_block_host(comp_len ? comp : comp + 1, comp_len, out, out_len, crc, 64, &lines);
    bool guards = true;
    for (uint32_t k = 0; k < kGuard; ++k) guards = guards && frame[k] == 0xA5 && out[out_len + k] == 0xA5;
    const uint32_t hash = verdict == CSI_OK ? adler32(out, out_len) : 0;
    printf("%u %u %u %u %d\n", i, verdict, hash, verdict == CSI_OK ? lines : 0, guards ? 1 : 0);
    // once more with the plain CRC: the two ways of forming it must agree on every text
    memset(frame, 0xA5, (size_t)out_len + 2 * kGuard);
    const uint32_t verdict1 = csi_inflate_block_host(comp_len ? comp : comp + 1, comp_len, out, out_len, crc, 1, &lines1);
    if (verdict1 != verdict || (verdict == CSI_OK && lines1 != lines)) {
      fprintf(stderr, "case %u: verdict %u with 64 CRC slices, %u with one\n", i, verdict, verdict1);
      return 2;
    }
    free(frame);
    free(comp);
  }
  fclose(fh);
  return 0;
}
