// Host-side parsers of everything the C ABI accepts as bytes or text: the iden3 binfile container,
// snarkjs .wtns, groth16 .zkey and circom .r1cs, the witness-program image written by
// zkfl/wprog.py, and circom's input.json.  Pure C++ (no HIP): libzkfl links it, and
// tools/parse_fuzz.cc and tools/r1cs_fuzz.cc link the same file under AddressSanitizer/UBSan for
// the corpus tests (tests/test_parse_fuzz.py, tests/test_r1cs_parse_cpu.py).
//
// Every reader checks a length before it reads: offsets are compared as `need > len - off` (never
// `off + need > len`, which wraps for a crafted 64-bit size), counts taken from a file are bounded
// before they size an allocation, and a failed check returns ZKFL_E_FORMAT / ZKFL_E_PRIME /
// ZKFL_E_MISMATCH / ZKFL_E_ARG with a message, leaving the outputs unspecified.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace zkfl {

// ---------------------------------------------------------------------------
// iden3 binfile: magic (4) | version u32 | nSections u32 | {type u32, size u64, data}*
// ---------------------------------------------------------------------------
struct Section {
  size_t off = 0, size = 0;
  bool present = false;
};
int binfile_sections(const uint8_t* buf, size_t len, const char magic[4], std::vector<Section>& secs,
                     std::string& err);

// .wtns v2: section 1 = n8 u32 | prime (n8 B) | nWitness u32; section 2 = nWitness x 32 B std
struct WtnsView {
  const uint8_t* data = nullptr;
  uint32_t n = 0;
};
int wtns_parse(const uint8_t* buf, size_t len, WtnsView& out, std::string& err);

// groth16 .zkey -> header, point sections, and the QAP coefficients as CSR rows (A rows then B
// rows over one term array) with the packed-dictionary encoding of csrc/poly.hip::k_abc_chunks.
struct ZkeyHost {
  uint32_t nVars = 0, nPub = 0, dom = 0;
  int logn = 0;
  size_t nC = 0;  // C query length nVars - nPub - 1
  const uint8_t* pts = nullptr;  // alpha1 64 | beta1 64 | beta2 128 | gamma2 128 | delta1 64 | delta2 128
  const uint8_t *secIC = nullptr, *secA = nullptr, *secB1 = nullptr, *secB2 = nullptr, *secC = nullptr, *secH = nullptr;
  size_t ncoef = 0;
  std::vector<uint32_t> rowptr;  // [2 (dom + 1)]: A row pointers, then B row pointers offset by nnz(A)
  std::vector<uint32_t> cols;    // packed terms (col | dict index << cshift) or plain columns
  std::vector<uint32_t> coefs;   // dictionary (packed) or one coefficient per term, 8 u32 each
  uint32_t cshift = 0;           // 0 = wide terms
};
int zkey_parse(const uint8_t* buf, size_t len, ZkeyHost& out, std::string& err);

// The A query in D form (csrc/key_load.hip): D_i = A_i - B1_i per wire, so that
// A = B1 + sum w_i D_i and a wire whose two bases are the same point (an S-box square: x * x = y)
// costs the A MSM nothing.  secA / secB1: n records of 64 B (affine, zeros = infinity); equality is
// byte equality.  Of the wires of this shard (i % nshards == shard) the D image keeps, in wire
// order, the pair (A_i, B1_i) as 128 B wherever the two records differ, with sidx = i; wires with
// equal records (both infinity included) are dropped.  On shard 0 the augmentation pairs follow
// (a null point = infinity).  The D form is used only when it has fewer bases than the A image
// would (its non-zero records of this shard + a_aug augmentation slots on shard 0).
struct AbAug {
  const uint8_t *p, *q;  // the pair's points, 64 B each (nullptr: infinity)
  uint32_t sidx;
};
struct AbPartition {
  bool d_form = false;
  size_t shared = 0;           // wires of this shard with equal non-zero records
  size_t n_a = 0, n_d = 0;     // bases of the A image / the D image (augmentation included)
  std::vector<uint8_t> img;    // [n_d x 128] when d_form, else empty
  std::vector<uint32_t> sidx;  // [n_d]
};
void ab_partition(const uint8_t* secA, const uint8_t* secB1, size_t n, uint32_t shard, uint32_t nshards,
                  const AbAug* aug, size_t n_aug, size_t a_aug, AbPartition& out);

// iden3 .r1cs v1 (the format zkfl/r1cs_file.py documents; it rejects what read_r1cs rejects):
// section 1 header, section 2 constraints, optional section 3 wire-to-label map of nWires x u64.
// With csr: the constraints as CSR rows over one term array -- the A rows, then the B rows, then
// the C rows, terms in file order (zero coefficients and repeated wires kept as they are) -- in
// zkey_parse's term encoding, coefficients std form as the file stores them.
struct R1csHost {
  uint32_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0, m = 0;
  uint64_t n_labels = 0, n_terms = 0;  // n_terms: every term of the file, < 2^32
  std::vector<uint32_t> rowptr;  // [3 m + 1]
  std::vector<uint32_t> cols;    // packed terms (col | dict index << cshift) or plain columns
  std::vector<uint32_t> coefs;   // dictionary (packed) or one coefficient per term, 8 u32 each
  uint32_t cshift = 0;           // 0 = wide terms
};
int r1cs_parse(const uint8_t* buf, size_t len, bool csr, R1csHost& out, std::string& err);

// snarkjs .ptau v1 (the layout zkfl/ptau.py documents; it rejects what its Ptau class rejects):
// sections 1-7 present, bn128's q, power 1..28, sections 2-6 of 2n-1 / n / n / n / 1 points
// (n = 2^power; G1 64 B, G2 128 B), sections 12-15 all present -- of 4n-1 / 2n-1 / 2n-1 / 2n-1
// points -- or all absent.  sec[t] / cnt[t]: section t's first byte and its point count (t = 2..6,
// 12..15; null / 0 for the Lagrange sections of an unprepared file).
struct PtauHost {
  uint32_t power = 0, ceremony_power = 0, contributions = 0;
  bool prepared = false;
  const uint8_t* sec[16] = {};
  size_t cnt[16] = {};
};
int ptau_parse(const uint8_t* buf, size_t len, PtauHost& out, std::string& err);

// ---------------------------------------------------------------------------
// Witness-program image (zkfl/wprog.py, "zkwp" v2)
// ---------------------------------------------------------------------------
enum : uint32_t { K_LC = 0, K_MUL = 1, K_INV = 2, K_BITS = 3, K_POS = 4 };
constexpr int MAX_T = 17;

struct WSignal {  // one declared input signal (input.json key)
  std::string name;
  std::vector<uint32_t> dims;
  uint32_t first = 0;
  uint32_t pub = 0;
};

struct PosWidthHost {
  uint32_t rp = 0, c_off = 0, m_off = 0;  // in Fr units within `consts`
};

// A validated image: the device code may trust every index in it.
struct WProgHost {
  uint32_t n_wires = 0, n_pub_out = 0, n_pub_in = 0, n_prv_in = 0, in_first = 0;
  uint32_t n_ops = 0, n_levels = 0, n_lcs = 0, n_terms = 0, n_asserts = 0, n_tmpl = 0;
  std::vector<uint32_t> level_ptr;
  const uint8_t *ops = nullptr, *lc_ptr = nullptr, *term_wire = nullptr, *term_coef = nullptr,
                *asserts = nullptr, *tmpl = nullptr;  // views into the image
  std::vector<uint8_t> consts;                         // Poseidon constants of every width used
  PosWidthHost width[MAX_T + 1];
  std::vector<WSignal> signals;
};
int wprog_parse(const uint8_t* img, size_t len, WProgHost& out, std::string& err);
// The signal table alone (zkfl_wprog_parse_inputs: no structural validation of the ops).
int wprog_signals(const uint8_t* img, size_t len, std::vector<WSignal>& out, std::string& err);

// circom's input.json -> flattened input signals (n_inputs x 8 u32 std form, reduced mod r).
int inputs_from_json(const std::vector<WSignal>& sigs, const char* json, std::vector<uint32_t>& out,
                     std::string& err);

// range checks of 8-limb little-endian values: v < r (scalar field), v < q (base field)
bool fr_lt_r(const uint32_t v[8]);
bool fq_lt_q(const uint32_t v[8]);

}  // namespace zkfl
