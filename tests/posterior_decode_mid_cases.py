"""Models, emissions, class maps and bounds shared by the tests of hmm_posterior_decode_mid (17..64 states):
tests/test_posterior_decode_mid_cpu.py checks every case's margin share on the fp64 oracle alone,
tests/test_posterior_decode_mid_gpu.py runs the same cases on the device.

Emissions are PEAKED, E = 0.05 + 0.9 u^4 with u uniform: with flat uniform emissions the posteriors of models of this
size are so even that more than 1 % of the positions lie within the fp32 posteriors' tolerance of a tie, and a label
comparison would say little."""
import functools

import numpy as np

import postgrad_mid_cases as pm
from test_engine_gpu import rand_model


def tol(n):
    """|conf - fp64 class sum of the engine's own gamma| for a largest class of n states: the bound of the q <= 16
    test, 2e-6 for 15 fp32 additions of terms that sum to <= 1 (15 * 2^-24 = 9e-7, doubled for the reference side),
    scaled with the number of additions."""
    return 2e-6 * max(1.0, (n - 1) / 15.0)


STATE_TOL = 2e-5                  # the posteriors' own tolerance against the fp64 oracle, per state (test_engine_gpu)
MARGIN_CAP = 0.01                 # share of a case's positions that may lie within 2 tol(n) of a tie
ORACLE_CAP = 0.02                 # ... within 2 n STATE_TOL of a tie on the oracle


def emissions(rng, k, b, L, q):
    return (0.05 + 0.9 * rng.random((k, b, L, q)) ** 4).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gene(q):
    A, pi = pm.gene_model(pm.copies_of(q))
    return np.array(A), np.array(pi)


def model(name, q, k, rng):
    """k models of q states -> A (k,q,q), pi (k,q): 'dense' (rand_model) or 'gene' (the (q - 1) / 14-copy gene model,
    every model with a start distribution of its own)."""
    if name == "gene":
        A = np.stack([gene(q)[0]] * k).astype(np.float32)
        pi = np.stack([gene(q)[1]] + [rand_model(rng, q)[1] for _ in range(k - 1)]).astype(np.float32)
        return A, pi
    A, pi = zip(*(rand_model(rng, q) for _ in range(k)))
    return np.stack(A), np.stack(pi)


def gene_classes(q):
    """intergenic, then five classes per copy's 14 states (3, 3, 3, 3, 2 of them), shared by the copies: 6 classes, the
    largest with 3 (q - 1) / 14 states (tests/test_posterior_decode_gpu.py::test_fallback_above_sixteen_states)."""
    return [0] + [1 + (i % 14) // 3 for i in range(q - 1)]


def largest_class(table, C):
    return int(np.bincount(np.asarray(table), minlength=C).max())


def random_map(rng, q, C, empty=()):
    """q class indices in 0..C-1, every class used except those of `empty`."""
    use = [c for c in range(C) if c not in empty]
    table = [use[i % len(use)] for i in range(q)]
    rng.shuffle(table)
    return [int(c) for c in table]


def class_cases():
    """-> list of (tag, model name, q, table, C, seed).  A case's inputs are model(name, q, k, rng) and
    emissions(rng, k, b, L, q) drawn in this order from default_rng(seed), for every shape of CLASS_SHAPES."""
    rng = np.random.default_rng(2)
    cases = [("gene%d-6" % q, "gene", q, gene_classes(q), 6, 100 + q) for q in (29, 43, 57)]
    for q, C in ((17, 5), (24, 16), (33, 6), (48, 16), (64, 16), (64, 5), (32, 1)):
        cases.append(("dense%d-%d" % (q, C), "dense", q, random_map(rng, q, C), C, 200 + q + C))
    cases.append(("dense40-empty", "dense", 40, random_map(rng, 40, 7, empty=(2, 5)), 7, 300))
    cases.append(("gene29-empty0", "gene", 29, [c + 1 for c in gene_classes(29)], 7, 301))
    return cases


CLASS_SHAPES = ((16, (2, 5, 333)), (48, (1, 17, 130)))          # (OPT_CHUNK, (k, b, L))


def class_inputs(case, shape):
    tag, name, q, table, C, seed = case
    k, b, L = shape
    rng = np.random.default_rng([seed, k, b, L])
    A, pi = model(name, q, k, rng)
    return A, pi, emissions(rng, k, b, L, q)


def oracle_cases():
    """-> list of (tag, model name, q, table or None, C, seed): one model, ORACLE_SHAPE."""
    rng = np.random.default_rng(4)
    return [("gene29-6", "gene", 29, gene_classes(29), 6, 401), ("gene43-ident", "gene", 43, None, 43, 402),
            ("dense24-4", "dense", 24, random_map(rng, 24, 4), 4, 403),
            ("dense64-16", "dense", 64, random_map(rng, 64, 16), 16, 404)]


ORACLE_SHAPE = (1, 4, 300)                                       # (64 states: the 64-lane scan)


def oracle_inputs(case):
    return class_inputs(case, ORACLE_SHAPE)
