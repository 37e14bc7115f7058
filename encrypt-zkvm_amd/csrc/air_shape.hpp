// air_shape.hpp -- ProcessorAir metadata shared by the prover and the verifier (host only).
#pragma once
#include <stddef.h>

#include <algorithm>

#include "../../include/zkvm_gpu.h"
#include "ext2.hpp"

namespace zk {
// num_constraint_composition_columns for the ProcessorAir transition degrees (air/src/lib.rs:69-90;
// winter-air TransitionConstraintDegree::get_evaluation_degree, cycle length 16) [DESIGN P6]:
// ceil((max evaluation degree - divisor degree) / n), divisor degree n - 2 (two exemptions)
// The declared degrees (TransitionConstraintDegree::new(base) / with_cycles(base, [16])): the evaluation degree of
// constraint k over a trace of n rows is base[k] (n - 1) + cyc[k] 15 n / 16.
struct DeclaredDegrees {
    int base[20], cyc[20];
    size_t evaluation_degree(int k, size_t n) const { return (size_t)base[k] * (n - 1) + (cyc[k] ? (n / 16) * 15 : 0); }
};
inline const DeclaredDegrees &air_declared_degrees() {
    static const DeclaredDegrees d = {{1, 5, 2, 6, 6, 6, 7, 7, 6, 6, 6, 6, 4, 7, 4, 4, 2, 2, 2, 2},
                                      {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1}};
    return d;
}
inline int num_comp_cols(size_t n) {
    const DeclaredDegrees &d = air_declared_degrees();
    size_t hi = 0;
    for (int k = 0; k < 20; k++) hi = std::max(hi, d.evaluation_degree(k, n));
    size_t c = (hi - (n - 2) + n - 1) / n;
    return (int)std::max<size_t>(c, 1);
}
// verifier.cpp: the out-of-domain constraint identity at z (ood = [T(z)]_W ++ [T(zg)]_W ++ [H_j(z)]_C;
// ct: 20 transition, cb: 22 boundary composition coefficients), over E (base values lift with b = 0)
bool ood_identity(const fe2 *ood, int C, const fe2 *ct, const fe2 *cb, fe2 z, size_t n, const zk_pub_inputs *pub);
// verifier.cpp: ProcessorAir::evaluate_transition (air/src/lib.rs:104-168) at one base-field frame -- the verifier's
// frame evaluator with every value lifted (b = 0); cur / nxt: the 28 cells of rows s and s + 1, per: the 9 periodic
// values of the step, out: the 20 constraint values.  air_periodic_row: row `step mod 16` of the raw periodic table
// (CYCLE_MASK || round constants, lib.rs:201-225).
void air_eval_base(const fe *cur, const fe *nxt, const fe *per, uint32_t lwe_size, uint32_t delta, fe *out);
void air_periodic_row(size_t step, fe out[9]);
}  // namespace zk
