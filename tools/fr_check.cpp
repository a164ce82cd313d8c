// Host-side driver for the 8 x 32-bit Montgomery field code (csrc/field.h) over Fr, used by
// tests/test_fr_mul_one.py: fp_add, fp_sub, fp_mul and the conversions are __host__ __device__ (on
// the host the column multiply-add is plain C++ instead of v_mad_u64_u32, the rest is the same
// code), so what the NTT's product-free butterflies rest on is checked on the CPU against Python
// big integers.  One operation per stdin line:
//   one | mul a b | mulone a | add a b | sub a b | tomont a | frommont a
// elements as 64 hex digits (big-endian, the whole 256-bit word: operands need not be reduced);
// the result is printed the same way.
// Build: hipcc --offload-arch=gfx950 -O1 -std=c++17 -I<pkg>/csrc -o fr_check fr_check.cpp
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "field.h"
using namespace zkfl;

static Fr rd(std::istringstream& in) {
  std::string t;
  in >> t;
  Fr r = fp_zero<FrP>();
  if (t.size() != 64) return r;
  for (int i = 0; i < 8; i++) r.v[7 - i] = (uint32_t)std::stoul(t.substr(8 * i, 8), nullptr, 16);
  return r;
}

static void wr(const Fr& a) {
  for (int i = 7; i >= 0; i--) printf("%08x", a.v[i]);
  printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op;
    in >> op;
    if (op == "one") wr(fp_one<FrP>());
    else if (op == "mul") { const Fr a = rd(in), b = rd(in); wr(fp_mul(a, b)); }
    else if (op == "mulone") wr(fp_mul(rd(in), fp_one<FrP>()));
    else if (op == "add") { const Fr a = rd(in), b = rd(in); wr(fp_add(a, b)); }
    else if (op == "sub") { const Fr a = rd(in), b = rd(in); wr(fp_sub(a, b)); }
    else if (op == "tomont") wr(fp_to_mont(rd(in)));
    else if (op == "frommont") wr(fp_from_mont(rd(in)));
    else return 1;
  }
  return 0;
}
