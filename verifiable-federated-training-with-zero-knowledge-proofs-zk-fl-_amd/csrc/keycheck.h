// The key check (csrc/keycheck.hip; zkfl_zkey_check): is a .zkey the Groth16 proving key of a
// resident .r1cs over a prepared .ptau, for some delta and gamma?  The reference trusts whatever
// `<c>_final.zkey` it finds (tests/full_system_simulation.mjs:713-738).
//
// Four stages on the context's stream (profiler names keycheck_points / _rows / _msm / _pairing):
//   points   k_points_check, one lane per point of the header and of sections 3, 5, 6, 7, 8, 9:
//            Montgomery coordinates < q, the curve equation, for G2 the order-r subgroup
//            (verify_dev.h g2_subgroup_criterion); count and lowest index reduced by wave ballot,
//            LDS and one atomic pair per workgroup, as k_r1cs_verdict does;
//   rows     the .r1cs rows on rho restricted to the public wires and to the rest (r1cs_check.h
//            r1cs_terms + abc_row, with the public rows a[m + s] += v[s]), their sum, the key's
//            section-4 rows on rho (poly.h abc_chunks) and k_rows_compare between the two;
//   msm      the one MSM engine (msm_api.h) over the key's sections and the ptau's Lagrange blocks,
//            scalars device-resident (the rows to std form in place), each block uploaded once;
//   pairing  k_key_finish compares the G1 / G2 sums of A, B1, B2 and writes the eight pairing
//            inputs, which go through verify.h pairing_batch; the GT values are compared pairwise.
// The point test, the verdict reduction and the comparison helpers are pointcheck.h's (shared with
// the ptau check).
#pragma once
