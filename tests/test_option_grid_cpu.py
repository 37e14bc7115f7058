"""The option grid of tests/option_grid.py, checked without a GPU: the table covers every (blowup, folding, extension)
triple with shapes the prover accepts, and the oracle's side of the small and over-folded cases is what
tests/test_gpu_option_grid.py expects the GPU to reproduce.  (The 32 oracle proofs of the grid run with the GPU tests.)
"""
import pytest

from option_grid import (BLOWUPS, EXTENSIONS, FOLDINGS, GRID, GRID_QUERIES, MAX_FRI_LAYERS, OVERFOLDED, SMALL,
                         SMALL_PROGRAMS, case_id, layer_sizes, options, oracle_options, small_trace)
from test_gpu_parity import oracle_pub
from zkvm_amd import native


def test_grid_covers_every_triple():
    assert len(GRID) == 32
    assert {(b, f, e) for b, f, e, _, _ in GRID} == {(b, f, e) for b in BLOWUPS for f in FOLDINGS for e in EXTENSIONS}


@pytest.mark.parametrize("case", GRID, ids=case_id)
def test_grid_row_shape(case):
    blowup, folding, _, log_n, rem = case
    N = blowup << log_n
    assert (rem + 1) & rem == 0 and rem <= 255
    sizes = layer_sizes(N, blowup, folding, rem)
    assert 1 <= len(sizes) - 1 <= MAX_FRI_LAYERS
    assert len(sizes) - 1 <= 10
    assert sizes[-1] >= blowup and sizes[-1] // blowup <= 256
    assert GRID_QUERIES < N


def test_grid_blowup_8_folding_16_has_three_layers():
    (case,) = [c for c in GRID if c[:3] == (8, 16, 1)]
    assert len(layer_sizes(8 << case[3], 8, 16, case[4])) - 1 == 3


@pytest.mark.parametrize("name", list(SMALL_PROGRAMS))
@pytest.mark.parametrize("case", SMALL, ids=case_id)
def test_small_cases_prove_and_verify_on_the_oracle(oracle, case, name):
    blowup, folding, ext, rem, queries = case
    trace, pub = small_trace(name)
    n = trace.shape[1]
    assert n == {"pushadd64": 64, "lr128": 128}[name] and queries < n * blowup
    sizes = layer_sizes(n * blowup, blowup, folding, rem)
    assert sizes[-1] >= blowup
    opub = oracle_pub(oracle, pub)
    rc, proof, rec, _ = oracle.prove_rc(trace, opub, oracle_options(oracle, options(*case)))
    assert rc == 0
    assert rec.num_fri_layers == len(sizes) - 1 and rec.remainder_len == sizes[-1] // blowup
    assert oracle.verify(proof, opub, 0) == (0, "")


def test_small_case_layer_counts():
    assert [len(layer_sizes(n * 64, 64, 2, 0)) - 1 for n in (64, 128)] == [6, 7]
    assert [len(layer_sizes(n * 64, 64, 16, 255)) - 1 for n in (64, 128)] == [0, 0]


@pytest.mark.parametrize("name", list(SMALL_PROGRAMS))
@pytest.mark.parametrize("case", OVERFOLDED, ids=case_id)
def test_overfolded_cases_are_degree_errors_on_the_oracle(oracle, case, name):
    """The layer rule folds below the blowup: the last layer is shorter than the blowup, the remainder has no
    coefficient, and the layer's interpolant cannot be of degree below 0."""
    blowup, folding, ext, rem, queries = case
    trace, pub = small_trace(name)
    sizes = layer_sizes(trace.shape[1] * blowup, blowup, folding, rem)
    assert 0 < sizes[-1] < blowup
    rc, _, rec, _ = oracle.prove_rc(trace, oracle_pub(oracle, pub), oracle_options(oracle, options(*case)))
    assert rc == native.ZK_ERR_DEGREE == -20
    assert rec.remainder_len == 0 and rec.num_fri_layers == len(sizes) - 1
