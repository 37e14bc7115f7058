"""Plain-integer reference of the back half of a proof, for tests/test_gpu_back_half.py, and of the composition stage
before it, for tests/test_gpu_composition.py (not a test module).

Everything after the constraint commitment, restated over Python integers mod p = 2^128 - 45 2^40 + 1 and, over the
quadratic extension E = F[X] / (X^2 - X - 1), over pairs (a, b) = a + b X:

  * Horner evaluation of a polynomial with base coefficients at a base or an E point (the OOD frame);
  * the DEEP quotient by synthetic division: A = sum alpha_i T_i, S = A + sum gamma_j H_j (over E the composition
    column H_j = P_2j + X P_2j+1), D = (S - S(z)) / (x - z) + (A - A(zg)) / (x - zg), n coefficients with D_{n-1} = 0;
  * the grinding search: BLAKE3(seed || nonce_le64), the trailing zero bits of its first little-endian u64, the
    smallest hit of a window;
  * BatchMerkleProof::get_root: the root rebuilt from opened rows, their positions and the serialized batch proof
    (u8 number of paths, per path u8 length and 32-byte digests: what verifier.cpp parses and wire.py cuts out);
  * one FRI layer: its rows, their Merkle root by pairwise merges, and the fold: per row the interpolant of the
    `fold` values over x_r <zeta> evaluated at alpha by Lagrange's formula (over E by components);
  * the composition stage: a polynomial's 8 n values over the CE coset in the evaluator's coset-major order, its
    segmentation into column polynomials, the assertion terms' quotient (f0 - f0(1)) / (x - 1) + (f1 - f1(c)) / (x - c)
    with its remainder flag, and the constraint root over the columns' LDE rows.

The hash is the CPU oracle's BLAKE3 (oracle.blake3, pinned against the specification by tests/test_blake3_pin.py);
tests/test_back_half_ref_cpu.py checks each part of this file against the oracle and the golden proofs.
"""
from operator import mul

P = 2**128 - 45 * 2**40 + 1
NO_NONCE = 2**64 - 1


# ---------------------------------------------------------------- E = F[X] / (X^2 - X - 1)
def e_add(x, y):
    return ((x[0] + y[0]) % P, (x[1] + y[1]) % P)


def e_sub(x, y):
    return ((x[0] - y[0]) % P, (x[1] - y[1]) % P)


def e_mul(x, y):
    """(a + b X)(c + d X) = (a c + b d) + (a d + b c + b d) X"""
    (a, b), (c, d) = x, y
    bd = b * d
    return ((a * c + bd) % P, (a * d + b * c + bd) % P)


def e_inv(x):
    """conjugate / norm: the conjugate of X is 1 - X, N(a + b X) = a^2 + a b - b^2"""
    a, b = x
    ni = pow((a * a + a * b - b * b) % P, P - 2, P)
    return ((a + b) * ni % P, -b * ni % P)


def e_pow(x, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = e_mul(r, x)
        x = e_mul(x, x)
        e >>= 1
    return r


# ---------------------------------------------------------------- evaluation
def horner(coeffs, x):
    """sum_k coeffs[k] x^k for integers mod p"""
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def horner_ext(coeffs, z):
    """the same at an E point z = (a, b); coeffs are base elements or E pairs"""
    acc = (0, 0)
    for c in reversed(coeffs):
        acc = e_mul(acc, z)
        acc = e_add(acc, c) if isinstance(c, tuple) else ((acc[0] + c) % P, acc[1])
    return acc


def powers(x, n):
    out = [1] * n
    for k in range(1, n):
        out[k] = out[k - 1] * x % P
    return out


def powers_ext(z, n):
    out = [(1, 0)] * n
    for k in range(1, n):
        out[k] = e_mul(out[k - 1], z)
    return out


def eval_with_powers(coeffs, pw):
    """Horner's value as the dot product with a power table (one reduction; many polynomials at one point)"""
    return sum(map(mul, coeffs, pw)) % P


def ood_frame(tpolys, cpolys, z, zg, ext):
    """[T(z)] ++ [T(zg)] ++ [H(z)] for base-coefficient polynomials; over E (z, zg pairs) a list of pairs"""
    n = len(tpolys[0])
    if ext == 1:
        pz, pg = powers(z, n), powers(zg, n)
        return ([eval_with_powers(t, pz) for t in tpolys] + [eval_with_powers(t, pg) for t in tpolys] +
                [eval_with_powers(c, pz) for c in cpolys])
    pz, pg = powers_ext(z, n), powers_ext(zg, n)
    za, zb = [v[0] for v in pz], [v[1] for v in pz]
    ga, gb = [v[0] for v in pg], [v[1] for v in pg]
    return ([(eval_with_powers(t, za), eval_with_powers(t, zb)) for t in tpolys] +
            [(eval_with_powers(t, ga), eval_with_powers(t, gb)) for t in tpolys] +
            [(eval_with_powers(c, za), eval_with_powers(c, zb)) for c in cpolys])


# ---------------------------------------------------------------- DEEP
def divide_out(f, c, ext):
    """(F(x) - F(c)) / (x - c) by synthetic division: the n coefficients (the top one 0) and the remainder F(c)"""
    n = len(f)
    if ext == 1:
        q = [0] * n
        acc = 0
        for k in range(n - 1, 0, -1):
            acc = (acc * c + f[k]) % P
            q[k - 1] = acc
        return q, (acc * c + f[0]) % P
    q = [(0, 0)] * n
    acc = (0, 0)
    for k in range(n - 1, 0, -1):
        acc = e_add(e_mul(acc, c), f[k])
        q[k - 1] = acc
    return q, e_add(e_mul(acc, c), f[0])


def deep_combine(tpolys, cpolys, alpha_t, alpha_c, ext):
    """the coefficients of A = sum alpha_i T_i and S = A + sum gamma_j H_j (over E: lists of pairs, and
    H_j = P_2j + X P_2j+1 of the base columns cpolys)"""
    if ext == 1:
        A = [sum(map(mul, alpha_t, col)) % P for col in zip(*tpolys)]
        S = [(a + sum(map(mul, alpha_c, col))) % P for a, col in zip(A, zip(*cpolys))]
        return A, S
    aa, ab = [v[0] for v in alpha_t], [v[1] for v in alpha_t]
    A = [(sum(map(mul, aa, col)) % P, sum(map(mul, ab, col)) % P) for col in zip(*tpolys)]
    # gamma (p0 + p1 X) with gamma = (c, d): (c p0 + d p1) + (d p0 + (c + d) p1) X, so each component of S is a
    # dot product of a row of base coefficients (test_back_half_ref_cpu checks this against e_mul term by term)
    ga = [g[t] for g in alpha_c for t in (0, 1)]
    gb = [v for g in alpha_c for v in (g[1], g[0] + g[1])]
    S = [((a[0] + sum(map(mul, ga, col))) % P, (a[1] + sum(map(mul, gb, col))) % P)
         for a, col in zip(A, zip(*cpolys))]
    return A, S


def deep_quotient(tpolys, cpolys, z, zg, alpha_t, alpha_c, ext):
    """D = (S - S(z)) / (x - z) + (A - A(zg)) / (x - zg): n coefficients (ints; over E pairs)"""
    A, S = deep_combine(tpolys, cpolys, alpha_t, alpha_c, ext)
    q1, _ = divide_out(S, z, ext)
    q2, _ = divide_out(A, zg, ext)
    if ext == 1:
        return [(x + y) % P for x, y in zip(q1, q2)]
    return [e_add(x, y) for x, y in zip(q1, q2)]


# ---------------------------------------------------------------- grinding
def nonce_zeros(blake3, seed, nonce):
    """trailing zero bits of the first little-endian u64 of BLAKE3(seed || nonce_le64) (64 for a zero word)"""
    head = int.from_bytes(blake3(seed + nonce.to_bytes(8, "little"))[:8], "little")
    return (head & -head).bit_length() - 1 if head else 64


def grind_hits(blake3, seed, start, count, bits):
    """every nonce of [start, start + count) that passes, ascending"""
    return [v for v in range(start, start + count) if nonce_zeros(blake3, seed, v) >= bits]


def grind(blake3, seed, start, count, bits):
    """the smallest passing nonce of the window, NO_NONCE (~0) when it has none"""
    for v in range(start, start + count):
        if nonce_zeros(blake3, seed, v) >= bits:
            return v
    return NO_NONCE


def zeros_table(blake3, seed, start, count):
    """nonce_zeros of every nonce of the window, hashed once for searches that share it"""
    return [nonce_zeros(blake3, seed, v) for v in range(start, start + count)]


def grind_in_table(table, start, count, bits):
    """grind() over the first `count` nonces of a window whose zeros_table is `table`"""
    for t in range(count):
        if table[t] >= bits:
            return start + t
    return NO_NONCE


def proof_query_seed(blake3, view, program_hash, stack_outputs):
    """The coin seed a proof ground its nonce on, replayed from the proof itself (view: wire.parse_proof's): the seed
    of the context and public-input elements, merged in turn with the trace root, the constraint root, the digests of
    the OOD trace frame and of the OOD constraint values, the FRI layer roots and the remainder commitment (drawing
    from the coin leaves its seed alone).  The proof's nonce must be the first of 1, 2, ... that passes on it."""
    def el(v):
        return int(v).to_bytes(16, "little")

    def body(name):
        at, width, ln = view.sections[name]
        return view.raw[at + width:at + width + ln]

    k = view.field_extension
    ctx = [view.trace_width << 16, view.trace_len, P % 2**64, P >> 64,
           (k << 16) | (view.fri_folding << 8) | view.fri_rem_max_deg, view.grinding, view.blowup, view.num_queries]
    seed = blake3(b"".join(map(el, ctx + list(program_hash)[:2] + list(stack_outputs)[:16])))
    coms = [view.commitments[i:i + 32] for i in range(0, len(view.commitments), 32)]
    states = body("ood_trace_states")[1:]  # after the frame-count byte: per column T_c(z) then T_c(zg)
    es = 16 * k
    tz = b"".join(states[2 * es * c:2 * es * c + es] for c in range(view.trace_width))
    tzg = b"".join(states[2 * es * c + es:2 * es * c + 2 * es] for c in range(view.trace_width))
    for d in coms[:2] + [blake3(tz + tzg), blake3(body("ood_evaluations"))] + coms[2:]:
        seed = blake3(seed + d)
    return seed


# ---------------------------------------------------------------- batch Merkle openings
def parse_batch_proof(proof):
    """the per-path digest lists of a serialized BatchMerkleProof; ValueError unless the bytes are exactly that"""
    if not proof:
        raise ValueError("empty batch proof")
    paths, o = [], 1
    for _ in range(proof[0]):
        if o >= len(proof):
            raise ValueError("truncated batch proof")
        k = proof[o]
        o += 1
        if o + 32 * k > len(proof):
            raise ValueError("truncated path")
        paths.append([proof[o + 32 * t:o + 32 * t + 32] for t in range(k)])
        o += 32 * k
    if o != len(proof):
        raise ValueError("trailing bytes after the batch proof")
    return paths


def batch_root(blake3, leaves, positions, proof, depth):
    """BatchMerkleProof::get_root: leaves[t] is the digest of the leaf at positions[t] (distinct positions, any
    order) of a tree of 2^depth leaves; returns the root the proof bytes rebuild, ValueError when they cannot"""
    if len(set(positions)) != len(positions) or len(leaves) != len(positions):
        raise ValueError("positions must be distinct, one leaf each")
    if any(not 0 <= i < 1 << depth for i in positions):
        raise ValueError("position out of range")
    at = dict(zip(positions, leaves))
    norm = sorted({i & ~1 for i in positions})
    paths = [list(p) for p in parse_batch_proof(proof)]
    if len(paths) != len(norm):
        raise ValueError("wrong number of paths")

    def take(i):
        if not paths[i]:
            raise ValueError("path too short")
        return paths[i].pop(0)

    nodes, nxt = {}, []
    for i, l in enumerate(norm):
        left = at[l] if l in at else take(i)
        right = at[l + 1] if l + 1 in at else take(i)
        k = ((1 << depth) + l) >> 1
        nodes[k] = blake3(left + right)
        nxt.append(k)
    for _ in range(1, depth):
        cur, nxt, i = nxt, [], 0
        while i < len(cur):
            node, sib = cur[i], cur[i] ^ 1
            if i + 1 < len(cur) and cur[i + 1] == sib:
                sd = nodes[sib]
                i += 1
            else:
                # the digest comes from the path at the node's index in this level's list, as MerkleTree::prove_batch
                # files it (the list shrinks as siblings merge, the path vectors do not move)
                sd = take(i)
            nodes[node >> 1] = blake3(sd + nodes[node]) if node & 1 else blake3(nodes[node] + sd)
            nxt.append(node >> 1)
            i += 1
    if any(paths):
        raise ValueError("unused digests in the batch proof")
    return nodes[1] if depth > 0 else None


def row_digest(blake3, row):
    """the leaf of an opened row: BLAKE3 over its elements' 16-byte encodings (row: ints or the bytes themselves)"""
    if isinstance(row, (bytes, bytearray)):
        return blake3(bytes(row))
    return blake3(b"".join(int(v).to_bytes(16, "little") for v in row))


# ---------------------------------------------------------------- one FRI layer
TWO_ADIC_ROOT = pow(3, (P - 1) >> 40, P)  # order 2^40; w_L = TWO_ADIC_ROOT^(2^40 / L)
FRI_OFFSET = 3


def fri_rows(layer, fold):
    """row r of a layer of L values (natural order): [layer[r + k L / fold]] for k < fold, the values at x_r zeta^k"""
    rows = len(layer) // fold
    return [[layer[r + k * rows] for k in range(fold)] for r in range(rows)]


def interp_eval(xs, vs, alpha, ext):
    """the polynomial of degree < len(xs) through (xs[k], vs[k]) (base points; base or E values), evaluated at alpha,
    by Lagrange's formula: the interpolation is F-linear, so over E it is taken by components"""
    inv = [pow(prod_mod(xs[k] - xs[j] for j in range(len(xs)) if j != k), P - 2, P) for k in range(len(xs))]
    if ext == 1:
        return sum(v * w % P * prod_mod(alpha - xs[j] for j in range(len(xs)) if j != k)
                   for k, (v, w) in enumerate(zip(vs, inv))) % P
    acc = (0, 0)
    for k, (v, w) in enumerate(zip(vs, inv)):
        num = (1, 0)
        for j in range(len(xs)):
            if j != k:
                num = e_mul(num, e_sub(alpha, (xs[j], 0)))
        acc = e_add(acc, e_mul(num, (v[0] * w % P, v[1] * w % P)))
    return acc


def prod_mod(values):
    r = 1
    for v in values:
        r = r * v % P
    return r


def fri_fold(layer, fold, alpha, ext):
    """the next layer: entry r is the interpolant of row r over x_r <zeta> at alpha, x_r = 3 w_L^r, zeta = w_fold"""
    L = len(layer)
    w = pow(TWO_ADIC_ROOT, (1 << 40) // L, P)
    zeta = pow(TWO_ADIC_ROOT, (1 << 40) // fold, P)
    zs = powers(zeta, fold)
    out, x = [], FRI_OFFSET
    for row in fri_rows(layer, fold):
        out.append(interp_eval([x * t % P for t in zs], row, alpha, ext))
        x = x * w % P
    return out


def fri_layer_root(blake3, layer, fold, ext):
    """the Merkle root over the rows' digests (a row's E values hashed as a, b per value), by pairwise merges"""
    level = [row_digest(blake3, row if ext == 1 else [c for v in row for c in v]) for row in fri_rows(layer, fold)]
    while len(level) > 1:
        level = [blake3(level[i] + level[i + 1]) for i in range(0, len(level), 2)]
    return level[0]


# ---------------------------------------------------------------- the composition stage
CE_BLOWUP = 8  # the constraint evaluation domain: 8 n points 3 w_8n^i
ASSERT_COL0 = [0, 7, 8, 11] + list(range(12, 20))  # the step 0 assertions' columns (coefficients 0 .. 11)
ASSERT_COL1 = [7, 8] + list(range(12, 20))  # the step n - 2 assertions' columns (coefficients 12 .. 21)


def composition_values(coeffs, n, eval_coset=None):
    """The 8 n values of the polynomial with the given (at most 8 n) coefficients over the CE coset, coset-major as
    the evaluator writes them: out[r n + q] = P(3 w_8n^r w_n^q) = P(3 w_8n^(r + 8 q)).  eval_coset: the oracle's
    transform (natural order) where its speed is wanted; without it every point by Horner's rule."""
    ce = CE_BLOWUP * n
    assert len(coeffs) <= ce
    if eval_coset is not None:
        nat = eval_coset(list(coeffs), ce, FRI_OFFSET)
    else:
        w = pow(TWO_ADIC_ROOT, (1 << 40) // ce, P)
        nat = [horner(coeffs, FRI_OFFSET * x % P) for x in powers(w, ce)]
    return [nat[r + CE_BLOWUP * q] for r in range(CE_BLOWUP) for q in range(n)]


def segment(coeffs, n, ncols):
    """the column polynomials: column c holds coefficients [c n, (c + 1) n), zeros past the end of coeffs"""
    full = list(coeffs) + [0] * max(0, ncols * n - len(coeffs))
    return [full[c * n:(c + 1) * n] for c in range(ncols)]


def boundary_quotient(tpolys, cb, bnd1, c):
    """The assertion terms' quotient of one coefficient plane: with f0 = sum_{i<12} cb[i] T_col0[i] and
    f1 = sum_{j<10} cb[12+j] T_col1[j] - bnd1, the n coefficients of (f0 - f0(1)) / (x - 1) + (f1 - f1(c)) / (x - c),
    and flag = 1 iff a remainder f0(1) or f1(c) is non-zero (an assertion fails).  The quotient is defined either way.
    Over the quadratic extension the coefficients cb and bnd1 are E values but the trace polynomials and both divisor
    points are base-field, so component j of the quotient is this function of component j of every cb and of bnd1: the
    planes are independent and the caller takes them one at a time (test_back_half_ref_cpu checks that against e_mul
    and the E division term by term)."""
    cols0, cols1 = [tpolys[k] for k in ASSERT_COL0], [tpolys[k] for k in ASSERT_COL1]
    f0 = [sum(map(mul, cb[:12], col)) % P for col in zip(*cols0)]
    f1 = [sum(map(mul, cb[12:22], col)) % P for col in zip(*cols1)]
    f1[0] = (f1[0] - bnd1) % P
    q0, r0 = divide_out(f0, 1, 1)
    q1, r1 = divide_out(f1, c, 1)
    return [(x + y) % P for x, y in zip(q0, q1)], int(r0 != 0 or r1 != 0)


def composition_root(blake3, merkle_root, eval_coset, polys, n, blowup):
    """The constraint commitment of the base columns `polys` (in column order: over E the components a, b of each E
    column): every column extended over the blowup n points 3 w_N^i by the oracle's transform, row i the columns'
    values there, each row hashed (row_digest) and the rows' Merkle root taken by the oracle."""
    ldes = [eval_coset(list(col), blowup * n, FRI_OFFSET) for col in polys]
    return merkle_root(b"".join(row_digest(blake3, row) for row in zip(*ldes)))
