"""tests/back_half_ref.py against the CPU oracle and the golden proofs (no GPU): the reference the GPU tests of the
OOD frame, the DEEP quotient, grinding and the batch openings compare with must not be wrong the way a kernel could be.
"""
import json
import random
from pathlib import Path

import pytest

import back_half_ref as ref
from zkvm_amd import wire

P = ref.P
GOLD = Path(__file__).resolve().parent / "golden"
CASES = {c["name"]: c for c in json.loads((GOLD / "cases.json").read_text())["cases"]}


def rand_e(rnd):
    return (rnd.randrange(P), rnd.randrange(P))


def test_horner_matches_oracle_coset_evaluation(oracle):
    rnd = random.Random(1)
    for n, offset in ((16, 1), (64, 3), (256, rnd.randrange(1, P))):
        coeffs = [rnd.randrange(P) for _ in range(n)]
        w = oracle.root_of_unity(n.bit_length() - 1)
        vals = oracle.eval_coset(coeffs, n, offset)
        xs = [offset * pow(w, i, P) % P for i in range(n)]
        assert [ref.horner(coeffs, x) for x in xs] == vals
        # the E evaluation at a lifted base point, and the power-table form of both
        assert [ref.horner_ext(coeffs, (x, 0)) for x in xs[:8]] == [(v, 0) for v in vals[:8]]
        assert [ref.eval_with_powers(coeffs, ref.powers(x, n)) for x in xs[:8]] == vals[:8]
    assert ref.horner([], 5) == 0 and ref.horner([7], 0) == 7 and ref.horner([1, 2, 3], 0) == 1


def test_extension_arithmetic_matches_oracle(oracle):
    rnd = random.Random(2)
    edge = [(0, 0), (1, 0), (0, 1), (P - 1, 0), (0, P - 1), (P - 1, P - 1), (1, 1)]
    xs = edge + [rand_e(rnd) for _ in range(40)]
    ys = list(reversed(edge)) + [rand_e(rnd) for _ in range(40)]
    for x, y in zip(xs, ys):
        assert ref.e_mul(x, y) == oracle.e2op("or_e2_mul", x, y), (x, y)
        if x != (0, 0):
            assert ref.e_inv(x) == oracle.e2op("or_e2_inv", x), x
            assert ref.e_mul(x, ref.e_inv(x)) == (1, 0)
    assert ref.e_mul((0, 1), (0, 1)) == (1, 1)  # X^2 = X + 1
    z = rand_e(rnd)
    assert ref.e_pow(z, 37) == ref.powers_ext(z, 38)[37]
    # horner_ext with E coefficients and with base coefficients against the power table
    n = 32
    base = [rnd.randrange(P) for _ in range(n)]
    pw = ref.powers_ext(z, n)
    want = (0, 0)
    for c, q in zip(base, pw):
        want = ref.e_add(want, ref.e_mul((c, 0), q))
    assert ref.horner_ext(base, z) == want
    assert ref.horner_ext([(c, 0) for c in base], z) == want
    frame = ref.ood_frame([base], [base], z, ref.e_mul(z, (3, 0)), 2)
    assert frame[0] == want and frame[2] == want and frame[1] == ref.horner_ext(base, ref.e_mul(z, (3, 0)))


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("n", [16, 64])
def test_deep_quotient_satisfies_the_pointwise_identity(oracle, n, ext):
    """D(x) (x - z)(x - zg) = (S(x) - S(z))(x - zg) + (A(x) - A(zg))(x - z) at every point of a coset, the
    polynomials evaluated there by the oracle; and D_{n-1} = 0."""
    rnd = random.Random(10 * n + ext)
    ccols = 3 * ext
    tp = [[rnd.randrange(P) for _ in range(n)] for _ in range(28)]
    cp = [[rnd.randrange(P) for _ in range(n)] for _ in range(ccols)]
    draw = (lambda: rnd.randrange(P)) if ext == 1 else (lambda: rand_e(rnd))
    z, zg = draw(), draw()
    at, ac = [draw() for _ in range(28)], [draw() for _ in range(ccols // ext)]
    D = ref.deep_quotient(tp, cp, z, zg, at, ac, ext)
    assert len(D) == n and D[n - 1] == (0 if ext == 1 else (0, 0))
    A, S = ref.deep_combine(tp, cp, at, ac, ext)
    # the combination term by term: A_k = sum alpha_i T_i[k], S_k = A_k + sum gamma_j (P_2j[k] + X P_2j+1[k])
    for k in (0, 1, n // 2, n - 1):
        if ext == 1:
            a = sum(x * t[k] for x, t in zip(at, tp)) % P
            s = (a + sum(x * c[k] for x, c in zip(ac, cp))) % P
        else:
            a = s = (0, 0)
            for x, t in zip(at, tp):
                a = ref.e_add(a, ref.e_mul(x, (t[k], 0)))
            s = a
            for j, x in enumerate(ac):
                s = ref.e_add(s, ref.e_mul(x, (cp[2 * j][k], cp[2 * j + 1][k])))
        assert (A[k], S[k]) == (a, s), k
    w = oracle.root_of_unity(n.bit_length() - 1)
    xs = [3 * pow(w, i, P) % P for i in range(n)]
    if ext == 1:
        Dx, Ax, Sx = (oracle.eval_coset(f, n, 3) for f in (D, A, S))
        Sz, Ag = ref.horner(S, z), ref.horner(A, zg)
        for x, d, a, s in zip(xs, Dx, Ax, Sx):
            assert d * (x - z) * (x - zg) % P == ((s - Sz) * (x - zg) + (a - Ag) * (x - z)) % P
    else:
        planes = lambda f: list(zip(oracle.eval_coset([v[0] for v in f], n, 3), oracle.eval_coset([v[1] for v in f], n, 3)))
        Dx, Ax, Sx = planes(D), planes(A), planes(S)
        Sz, Ag = ref.horner_ext(S, z), ref.horner_ext(A, zg)
        for x, d, a, s in zip(xs, Dx, Ax, Sx):
            xz, xg = ref.e_sub((x, 0), z), ref.e_sub((x, 0), zg)
            lhs = ref.e_mul(ref.e_mul(d, xz), xg)
            rhs = ref.e_add(ref.e_mul(ref.e_sub(s, Sz), xg), ref.e_mul(ref.e_sub(a, Ag), xz))
            assert lhs == rhs
    # the division is exact also where the point-wise quotient is not defined: z on the trace domain
    if ext == 1:
        q, r = ref.divide_out(S, w, 1)
        assert r == ref.horner(S, w)
        back = [(q[k - 1] if k else 0) - w * q[k] for k in range(n)]
        assert [(b + (r if k == 0 else 0)) % P for k, b in enumerate(back)] == S


@pytest.mark.parametrize("name", ["lr", "lr_f16_r15", "cipher8_quad_f2_g9"])
def test_batch_checker_rebuilds_a_golden_trace_root(oracle, name):
    c = CASES[name]
    proof = (GOLD / f"{name}.proof").read_bytes()
    view, _ = wire.parse_proof(proof)

    def body(section):
        at, width, ln = view.sections[section]
        return view.raw[at + width:at + width + ln]

    pos = c["positions"]
    depth = (c["trace_len"] * c["options"]["blowup"]).bit_length() - 1
    values, bproof = body("trace_values"), body("trace_proof")
    assert len(values) == len(pos) * 28 * 16
    leaves = [ref.row_digest(oracle.blake3, values[448 * q:448 * q + 448]) for q in range(len(pos))]
    assert ref.batch_root(oracle.blake3, leaves, pos, bproof, depth).hex() == c["trace_root"]
    # the same leaves in another order (the checker takes positions in any order)
    order = list(range(len(pos)))
    random.Random(3).shuffle(order)
    assert ref.batch_root(oracle.blake3, [leaves[i] for i in order], [pos[i] for i in order], bproof,
                          depth).hex() == c["trace_root"]
    # a changed row, a changed digest and a moved position rebuild another root; cut or padded bytes are refused
    bad_row = bytearray(values[:448])
    bad_row[5] ^= 1
    assert ref.batch_root(oracle.blake3, [ref.row_digest(oracle.blake3, bad_row)] + leaves[1:], pos, bproof,
                          depth).hex() != c["trace_root"]
    flipped = bytearray(bproof)
    flipped[len(bproof) // 2] ^= 1
    try:
        assert ref.batch_root(oracle.blake3, leaves, pos, bytes(flipped), depth).hex() != c["trace_root"]
    except ValueError:
        pass  # the flipped byte was a length
    for broken in (bproof[:-1], bproof + b"\0"):
        with pytest.raises(ValueError):
            ref.batch_root(oracle.blake3, leaves, pos, broken, depth)
    with pytest.raises(ValueError):
        ref.batch_root(oracle.blake3, leaves + leaves[:1], pos + pos[:1], bproof, depth)
    # the constraint rows of the same proof against the recorded constraint root
    cvals, cproof = body("constraint_values"), body("constraint_proof")
    rowb = len(cvals) // len(pos)
    cleaves = [ref.row_digest(oracle.blake3, cvals[rowb * q:rowb * q + rowb]) for q in range(len(pos))]
    assert ref.batch_root(oracle.blake3, cleaves, pos, cproof, depth).hex() == c["constraint_root"]


def test_batch_checker_on_a_small_tree(oracle):
    """Every pair of positions of an 8-leaf tree, the proof written here from the full tree."""
    b3 = oracle.blake3
    leaves = [b3(bytes([i])) for i in range(8)]
    lvl, tree = leaves, {}
    size = 8
    for i, d in enumerate(leaves):
        tree[8 + i] = d
    while size > 1:
        size //= 2
        for i in range(size):
            tree[size + i] = b3(tree[2 * (size + i)] + tree[2 * (size + i) + 1])
    assert tree[1] == oracle.merkle_root(b"".join(leaves))
    # {2, 3}: one path holding the pair's uncle and the other half's root
    proof = bytes([1, 2]) + tree[4] + tree[3]
    assert ref.batch_root(b3, [leaves[3], leaves[2]], [3, 2], proof, 3) == tree[1]
    # {0, 7}: two paths, each its leaf sibling and its uncle; the top level merges the two
    proof = bytes([2, 2]) + leaves[1] + tree[5] + bytes([2]) + leaves[6] + tree[6]
    assert ref.batch_root(b3, [leaves[0], leaves[7]], [0, 7], proof, 3) == tree[1]
    with pytest.raises(ValueError):
        ref.batch_root(b3, [leaves[0], leaves[7]], [0, 7], proof[:-32], 3)


@pytest.mark.parametrize("ext", [1, 2])
@pytest.mark.parametrize("fold", [2, 4, 8, 16])
def test_fri_fold_matches_oracle_interpolation(oracle, fold, ext):
    """Every row of a layer: the oracle interpolates the row's `fold` values over the coset x_r <zeta> (per component
    over E) and Horner's rule evaluates the coefficients at alpha."""
    rnd = random.Random(100 * fold + ext)
    L = 8 * fold
    draw = (lambda: rnd.randrange(P)) if ext == 1 else (lambda: rand_e(rnd))
    layer = [draw() for _ in range(L)]
    w = oracle.root_of_unity(L.bit_length() - 1)
    assert w == pow(ref.TWO_ADIC_ROOT, (1 << 40) // L, P)
    for alpha in (draw(), 0 if ext == 1 else (0, 0), 1 if ext == 1 else (0, 1)):
        got = ref.fri_fold(layer, fold, alpha, ext)
        assert len(got) == L // fold
        for r, row in enumerate(ref.fri_rows(layer, fold)):
            x = 3 * pow(w, r, P) % P
            if ext == 1:
                assert got[r] == ref.horner(oracle.interp_coset(row, x), alpha), (r, alpha)
            else:
                ca, cb = oracle.interp_coset([v[0] for v in row], x), oracle.interp_coset([v[1] for v in row], x)
                assert got[r] == ref.horner_ext(list(zip(ca, cb)), alpha), (r, alpha)
    # a row's points are x_r zeta^k: the values of X^m there interpolate back to alpha^m
    zeta = oracle.root_of_unity(fold.bit_length() - 1)
    xs = [3 * pow(zeta, k, P) % P for k in range(fold)]
    a = rnd.randrange(P)
    assert ref.interp_eval(xs, [pow(x, fold - 1, P) for x in xs], a, 1) == pow(a, fold - 1, P)


@pytest.mark.parametrize("name", ["pushadd12", "cipher8_b16_f4", "pushadd12_f2_r7", "lr_f16_r15"])
def test_fri_fold_reproduces_an_oracle_proofs_first_layer(oracle, name):
    """Folding the DEEP evaluations an oracle proof dumps at the recorded first alpha gives the first folded layer it
    dumps, and the layer's root is the recorded one (base field: the dump carries only the a component over E)."""
    import numpy as np

    c = CASES[name]
    trace = np.load(GOLD / f"{name}.trace.npy", allow_pickle=False)
    ints = lambda hs: [int(h, 16) for h in hs]
    pub = oracle.make_pub(ints(c["program_hash"]), ints(c["stack_outputs"]), c["lwe_size"], c["delta"])
    _, rec, dumps = oracle.prove(trace, pub, oracle.default_options(**c["options"]), want=("deep", "fri_layer1"))
    assert rec.num_fri_layers >= 1 and c["options"]["field_extension"] == 1
    fold = c["options"]["fri_folding"]
    val = lambda a: [int(lo) | int(hi) << 64 for lo, hi in a]
    deep, layer1 = val(dumps["deep"]), val(dumps["fri_layer1"])
    alpha = int.from_bytes(bytes(rec.fri_alphas)[:16], "little")
    assert ref.fri_fold(deep, fold, alpha, 1) == layer1
    assert ref.fri_layer_root(oracle.blake3, deep, fold, 1) == bytes(rec.fri_roots)[:32]


@pytest.mark.parametrize("name", ["lr_grind10_q28", "cipher8_quad_f2_g9"])
def test_grinding_reference_finds_the_golden_nonce(oracle, name):
    """The seed a golden proof ground on, replayed from the proof's own sections: the reference's search from 1
    upward returns the proof's pow_nonce, and no window before it holds a hit."""
    c = CASES[name]
    bits = c["options"]["grinding"]
    view, _ = wire.parse_proof((GOLD / f"{name}.proof").read_bytes())
    nonce = c["pow_nonce"]
    assert view.pow_nonce == nonce > 1 and view.grinding == bits
    seed = ref.proof_query_seed(oracle.blake3, view, [int(h, 16) for h in c["program_hash"]],
                                [int(h, 16) for h in c["stack_outputs"]])
    assert ref.grind(oracle.blake3, seed, 1, 4096, bits) == nonce
    assert ref.grind(oracle.blake3, seed, 1, nonce - 1, bits) == ref.NO_NONCE
    assert ref.grind_hits(oracle.blake3, seed, 1, nonce, bits) == [nonce]
    assert ref.nonce_zeros(oracle.blake3, seed, nonce) >= bits
    assert ref.grind(oracle.blake3, seed, nonce, 1, bits) == nonce and ref.grind(oracle.blake3, seed, 1, 1, 0) == 1
    assert ref.grind(oracle.blake3, seed, 1, 64, 64) == ref.NO_NONCE


# ---------------------------------------------------------------- the composition stage
def test_composition_values_by_horner_and_by_the_oracles_transform_agree(oracle):
    rnd = random.Random(21)
    n = 16
    full = [rnd.randrange(P) for _ in range(8 * n)]
    for coeffs in (full, full[:7 * n], [5], [0] * (7 * n) + [1], [P - 1] * (7 * n)):
        assert ref.composition_values(coeffs, n) == ref.composition_values(coeffs, n, oracle.eval_coset)
    # the layout: entry r n + q is the value at 3 w_8n^r w_n^q
    vals = ref.composition_values(full, n)
    w8n, wn = oracle.root_of_unity(7), oracle.root_of_unity(4)
    for r, q in ((0, 0), (1, 0), (0, 1), (7, 15), (3, 9)):
        assert vals[r * n + q] == ref.horner(full, 3 * pow(w8n, r, P) * pow(wn, q, P) % P)
    # and back: the natural-order values interpolate to the coefficients, which segment() cuts into columns
    nat = [vals[(i % 8) * n + i // 8] for i in range(8 * n)]
    assert oracle.interp_coset(nat, 3) == full
    assert ref.segment(full, n, 8) == [full[c * n:(c + 1) * n] for c in range(8)]
    assert ref.segment([1, 2, 3], 2, 3) == [[1, 2], [3, 0], [0, 0]] and ref.segment([1, 2, 3], 2, 1) == [[1, 2]]


def cross_step_model(oracle, comp, n, ncols, nce):
    """The cross-coset step in plain integers, as k_comp_cross is written: from the per-coset interpolants c_r, per k1
    the values d_r = c_r[k1] w_8n^(-r k1), with nce = 7 the derived d_7 = -sum_{r<7} w_8^(r+1) d_r, the size-8 transform
    b_k2 = sum_r w_8^(-r k2) d_r and a[k1 + n k2] = b_k2 3^-(k1 + n k2) / 8.  -> (ncols columns, top-block flag)"""
    w8n, w8 = oracle.root_of_unity((8 * n).bit_length() - 1), oracle.root_of_unity(3)
    c = [oracle.interp_coset(comp[r * n:(r + 1) * n], 1) for r in range(nce)]
    cols, flag = [[0] * n for _ in range(ncols)], 0
    for k1 in range(n):
        d = [c[r][k1] * pow(w8n, -r * k1, P) % P for r in range(nce)]
        if nce == 7:
            d.append(-sum(pow(w8, r + 1, P) * d[r] for r in range(7)) % P)
        for k2 in range(8):
            b = sum(pow(w8, -r * k2, P) * d[r] for r in range(8)) % P
            a = b * pow(8 * pow(3, k1 + n * k2, P), -1, P) % P
            if k2 < ncols:
                cols[k2][k1] = a
            else:
                flag |= a != 0
    return cols, int(flag)


def test_cross_step_with_a_derived_coset_model(oracle):
    """What tests/test_gpu_composition.py expects of the derived coset: for degree < 7n the polynomial itself, coset 7
    never read; for degree in [7n, 8n) a polynomial with a zero top block that agrees with the input on cosets 0 .. 6
    (flag 0); and with all eight cosets the flag is set exactly by a coefficient at or past ncols n."""
    rnd = random.Random(23)
    n = 16
    for coeffs in ([rnd.randrange(P) for _ in range(7 * n)], [0] * (7 * n - 1) + [1], [P - 1] * (7 * n), [P - 1]):
        vals = ref.composition_values(coeffs, n)
        hidden = vals[:7 * n] + [P - 1] * n
        assert cross_step_model(oracle, hidden, n, 7, 7) == (ref.segment(coeffs, n, 7), 0)
        assert cross_step_model(oracle, vals, n, 7, 8) == (ref.segment(coeffs, n, 7), 0)
    for coeffs in ([0] * (7 * n) + [1], [rnd.randrange(P) for _ in range(8 * n)]):
        vals = ref.composition_values(coeffs, n)
        cols, flag = cross_step_model(oracle, vals[:7 * n] + [P - 1] * n, n, 7, 7)
        q = [v for col in cols for v in col]
        assert flag == 0 and q != coeffs[:7 * n]
        assert ref.composition_values(q, n)[:7 * n] == vals[:7 * n]
        assert cross_step_model(oracle, vals, n, 7, 8) == (ref.segment(coeffs, n, 7), 1)
    for ncols in (1, 5):
        for k, want in ((ncols * n - 1, 0), (ncols * n, 1), (7 * n - 1, 1)):
            coeffs = [0] * k + [1]
            vals = ref.composition_values(coeffs, n)
            assert cross_step_model(oracle, vals, n, ncols, 7) == (ref.segment(coeffs, n, ncols), want)


def test_boundary_quotient_planes_are_the_extension_quotients_components():
    """The quotient over E, term by term with e_mul and divided at the lifted base points, is plane by plane the
    base-field quotient of that plane's coefficients; a remainder in either plane alone raises that plane's flag."""
    rnd = random.Random(22)
    n = 16
    tp = [[rnd.randrange(P) for _ in range(n)] for _ in range(28)]
    cb = [[rnd.randrange(P) for _ in range(22)] for _ in range(2)]
    bnd1 = [rnd.randrange(P) for _ in range(2)]
    c = pow(pow(ref.TWO_ADIC_ROOT, (1 << 40) // n, P), n - 2, P)
    cbe = list(zip(*cb))
    f0 = [(0, 0)] * n
    f1 = [(0, 0)] * n
    for k in range(n):
        for i, col in enumerate(ref.ASSERT_COL0):
            f0[k] = ref.e_add(f0[k], ref.e_mul(cbe[i], (tp[col][k], 0)))
        for j, col in enumerate(ref.ASSERT_COL1):
            f1[k] = ref.e_add(f1[k], ref.e_mul(cbe[12 + j], (tp[col][k], 0)))
    f1[0] = ref.e_sub(f1[0], tuple(bnd1))
    q0, r0 = ref.divide_out(f0, (1, 0), 2)
    q1, r1 = ref.divide_out(f1, (c, 0), 2)
    planes = [ref.boundary_quotient(tp, cb[j], bnd1[j], c) for j in range(2)]
    assert [ref.e_add(x, y) for x, y in zip(q0, q1)] == list(zip(planes[0][0], planes[1][0]))
    assert [int(r0[j] != 0 or r1[j] != 0) for j in range(2)] == [planes[0][1], planes[1][1]] == [1, 1]
    # remainders removed in plane 0 alone (its f0(1) through column 0's constant, its f1(c) through bnd1)
    s0 = sum(cb[0][i] * sum(tp[col]) for i, col in enumerate(ref.ASSERT_COL0)) % P
    tp[0][0] = (tp[0][0] - s0 * pow(cb[0][0], -1, P)) % P
    good1 = sum(cb[0][12 + j] * ref.horner(tp[col], c) for j, col in enumerate(ref.ASSERT_COL1)) % P
    q, flag = ref.boundary_quotient(tp, cb[0], good1, c)
    assert flag == 0 and q[n - 1] == 0
    assert ref.boundary_quotient(tp, cb[1], bnd1[1], c)[1] == 1
    assert ref.boundary_quotient(tp, cb[0], (good1 + 1) % P, c)[1] == 1


@pytest.mark.parametrize("name", ["lr", "lr_quad"])
def test_composition_reference_on_a_golden_workload(oracle, name):
    """The oracle's dumps of a golden workload: the composition values interpolate and segment into the column
    polynomials it commits to (over E the dump carries the a plane), whose root by composition_root is the recorded
    constraint root; and the boundary quotient of the trace polynomials under the recorded coefficients, evaluated at
    every CE point, is the point-wise f0(x) / (x - 1) + f1(x) / (x - c), with no remainder."""
    import numpy as np

    c = CASES[name]
    trace = np.load(GOLD / f"{name}.trace.npy", allow_pickle=False)
    ints = lambda hs: [int(h, 16) for h in hs]  # noqa: E731
    pub = oracle.make_pub(ints(c["program_hash"]), ints(c["stack_outputs"]), c["lwe_size"], c["delta"])
    opts = c["options"]
    _, rec, dumps = oracle.prove(trace, pub, oracle.default_options(**opts), want=("composition", "comp_polys"))
    n, K, ncols = c["trace_len"], opts["field_extension"], rec.num_ccols
    assert ncols == 7
    comp = oracle.array_to_elems(dumps["composition"])
    coeffs = oracle.interp_coset(comp, 3)
    assert not any(coeffs[ncols * n:])
    cpolys = oracle.array_to_elems(dumps["comp_polys"])[:ncols * K * n]
    base_cols = [cpolys[i * n:(i + 1) * n] for i in range(ncols * K)]
    assert ref.segment(coeffs, n, ncols) == base_cols[::K]
    assert ref.composition_values(coeffs, n, oracle.eval_coset) == [comp[r + 8 * q] for r in range(8) for q in range(n)]
    assert ref.composition_root(oracle.blake3, oracle.merkle_root, oracle.eval_coset, base_cols, n,
                                opts["blowup"]) == bytes(rec.constraint_root)
    # the assertion quotient (the record keeps the a component of every coefficient: plane a)
    tp = [oracle.interp_coset(oracle.array_to_elems(trace[k]), 1) for k in range(28)]
    cb = oracle.from_bytes(bytes(rec.coeff_b))[:22]
    asserted = ints(c["program_hash"])[:2] + ints(c["stack_outputs"])[:8]
    bnd1 = sum(x * v for x, v in zip(cb[12:], asserted)) % P
    g = oracle.root_of_unity(n.bit_length() - 1)
    cc = pow(g, n - 2, P)
    q, flag = ref.boundary_quotient(tp, cb, bnd1, cc)
    assert flag == 0 and q[n - 1] == 0 and any(q)
    ev = {k: oracle.eval_coset(tp[k], 8 * n, 3) for k in ref.ASSERT_COL0}
    w = oracle.root_of_unity((8 * n).bit_length() - 1)
    x = 3
    for i in range(8 * n):
        f0 = sum(cb[t] * ev[k][i] for t, k in enumerate(ref.ASSERT_COL0))
        f1 = sum(cb[12 + t] * ev[k][i] for t, k in enumerate(ref.ASSERT_COL1)) - bnd1
        want = (f0 * pow(x - 1, -1, P) + f1 * pow(x - cc, -1, P)) % P
        assert ref.horner(q, x) == want, i
        x = x * w % P
