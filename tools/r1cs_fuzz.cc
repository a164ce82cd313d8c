// Corpus driver for the .r1cs parser of libzkfl (csrc/host_parse.cc r1cs_parse, behind
// zkfl_r1cs_parse / zkfl_r1cs_load), built for the CPU under AddressSanitizer + UBSan by
// tests/test_r1cs_parse_cpu.py:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I include -I <pkg>/csrc tools/r1cs_fuzz.cc <pkg>/csrc/host_parse.cc -o r1cs_fuzz
//   r1cs_fuzz <corpus>
// The corpus is the test's own (well-formed files and their mutations, each with the verdict of
// zkfl/r1cs_file.py's read_r1cs): u32 count, then per case u8 accept | u64 len | bytes.  Every case
// runs from a private heap copy of exactly its length, header-only and with the CSR build; the
// parser must accept exactly the cases read_r1cs accepts, and an accepted file's CSR must be
// well-formed (monotone row pointers ending at the term count, columns below nWires, dictionary
// indices inside the dictionary).  -DZK_COEF_DICT_MAX=<small> builds the wide-term path.  The
// sanitizers abort on any out-of-bounds read, overflow or undefined behaviour; a clean run prints
// the number of cases and exits 0.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "host_parse.h"

using namespace zkfl;

static bool csr_ok(const R1csHost& h) {
  const size_t rows = 3 * (size_t)h.m;
  if (h.rowptr.size() != rows + 1 || h.rowptr[0] != 0 || h.rowptr[rows] != h.n_terms) return false;
  for (size_t r = 0; r < rows; r++)
    if (h.rowptr[r] > h.rowptr[r + 1]) return false;
  if (h.cols.size() != h.n_terms) return false;
  const uint32_t cmask = h.cshift ? (1u << h.cshift) - 1u : 0xFFFFFFFFu;
  const size_t ncoef = h.coefs.size() / 8;
  if (!h.cshift && ncoef != h.n_terms) return false;
  for (uint32_t t : h.cols) {
    if ((t & cmask) >= h.n_wires) return false;
    if (h.cshift && (t >> h.cshift) >= ncoef) return false;
  }
  for (size_t i = 0; i < ncoef; i++)
    if (!fr_lt_r(&h.coefs[8 * i])) return false;
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <corpus>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  uint32_t count = 0;
  if (!f || fread(&count, 4, 1, f) != 1) {
    fprintf(stderr, "unreadable corpus\n");
    return 2;
  }
  size_t accepted = 0;
  for (uint32_t i = 0; i < count; i++) {
    uint8_t want = 0;
    uint64_t len = 0;
    if (fread(&want, 1, 1, f) != 1 || fread(&len, 8, 1, f) != 1 || len > (1ull << 30)) return 2;
    std::vector<uint8_t> data((size_t)len);
    if (len && fread(data.data(), 1, (size_t)len, f) != len) return 2;
    data.shrink_to_fit();  // exactly len bytes on the heap: ASan sees every overread
    const uint8_t* p = data.empty() ? nullptr : data.data();
    for (int csr = 0; csr < 2; csr++) {
      R1csHost h;
      std::string err;
      const int rc = r1cs_parse(p, data.size(), csr != 0, h, err);
      if ((rc == 0) != (want != 0)) {
        fprintf(stderr, "case %u (csr %d): parser returned %d (%s), read_r1cs %s\n", i, csr, rc, err.c_str(),
                want ? "accepts" : "rejects");
        return 3;
      }
      if (rc > 0 || (rc < 0 && err.empty())) return 3;
      if (rc == 0 && csr && !csr_ok(h)) {
        fprintf(stderr, "case %u: malformed CSR\n", i);
        return 3;
      }
    }
    accepted += want != 0;
  }
  fclose(f);
  printf("r1cs_fuzz: %u cases (%zu accepted), no sanitizer findings\n", count, accepted);
  return 0;
}
