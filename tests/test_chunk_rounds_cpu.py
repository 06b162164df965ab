"""The round-aware chunk rule of the <= 16-state plans, without a device: hmm_chunk_len against a Python restatement
of the rule before it (choose_T) wherever the new rule must not engage, the engaged shapes against the restated cost
model, and the chunk-length queries of the other plans against values recorded at the commit before the rule."""
import itertools

import pytest

from hmm_layer_amd import build as hbuild
from hmm_layer_amd import engine

MAX_T = 512
CUS, APPLY_BPC, REDUCE_BPC = 256, 2, 4
STEP_W = 800


@pytest.fixture(scope="module")
def lib():
    hbuild.build()
    return engine.lib()


def floor_T(L):
    tb = 16
    while tb * tb * tb * 4 < 9 * L and tb < MAX_T:
        tb += 16
    return tb


def choose_T_old(NB, L):
    """hmm_chunk_len before the rule: enough chunks for 32 768 (sequence, chunk) pairs, never below T^3 = 2.25 L,
    a multiple of 16 in [16, 512], no longer than the sequence."""
    t = max(NB * L // 32768, floor_T(L))
    t = (t + 15) // 16 * 16
    t = min(max(t, 16), MAX_T)
    return min(t, (L + 15) // 16 * 16)


def chunks(L, T):
    return (L + T - 1) // T


def apply_blocks(k, b, L, T):
    return (k * ((b * chunks(L, T) + 15) // 16) + 3) // 4


def cost(k, b, L, T):
    """T steps per block the fullest compute unit serves, plus 1/800 step per chunk operator."""
    return STEP_W * ((apply_blocks(k, b, L, T) + CUS - 1) // CUS) * T + k * b * chunks(L, T)


def rule(k, b, L):
    t0 = choose_T_old(k * b, L)
    if t0 != MAX_T or k * b * chunks(L, t0) <= 64 * CUS * APPLY_BPC:
        return t0
    best = t0
    for t in range(t0 - 16, max(floor_T(L), t0 // 2) - 1, -16):
        if cost(k, b, L, t) < cost(k, b, L, best):
            best = t
    return best


GRID = [(1, 4, 128, 3), (1, 256, 10000, 15), (1, 128, 100000, 15), (2, 3, 17, 7)] + [
    (k, b, L, q) for k, b, L, q in itertools.product((1, 2, 3), (1, 5, 16, 100, 512, 1365, 2048, 10922),
                                                     (1, 17, 500, 512, 513, 8192, 9999, 100000, 1000000),
                                                     (1, 3, 7, 15, 16))]


def test_capacity_constants(lib):
    assert engine.plan_capacity() == dict(cus=CUS, forward_blocks_per_cu=APPLY_BPC, backward_blocks_per_cu=APPLY_BPC,
                                          reduce_blocks_per_cu=REDUCE_BPC)
    assert lib.hmm_plan_capacity(4) == -6 and lib.hmm_plan_capacity(-1) == -6        # HMM_ERR_BAD_ARGUMENT


def test_unengaged_shapes_keep_the_old_chunk(lib):
    seen = 0
    for k, b, L, q in GRID:
        t_old = choose_T_old(k * b, L)
        if k * b * chunks(L, t_old) > 32768:
            continue
        seen += 1
        assert lib.hmm_chunk_len(k, b, L, q) == t_old, (k, b, L, q)
    assert seen > 500
    # one round exactly, k = 3 with ragged waves per model: 32 766 chains, 513 blocks, still the old chunk
    assert choose_T_old(3 * 10922, 512) == 512 and lib.hmm_chunk_len(3, 10922, 512, 15) == 512


@pytest.mark.parametrize("dims", [(1, 1024, 100000, 15), (1, 2048, 8200, 3), (1, 4096, 9999, 15)])
def test_engaged_shapes(lib, dims):
    k, b, L, q = dims
    t_old = choose_T_old(k * b, L)
    assert t_old == MAX_T and k * b * chunks(L, t_old) > 32768
    T = lib.hmm_chunk_len(*dims)
    assert T % 16 == 0 and t_old // 2 <= T <= t_old
    assert cost(k, b, L, T) <= cost(k, b, L, t_old)
    assert T == rule(k, b, L)


def test_headline_shape_fills_whole_compute_units(lib):
    # 3584 blocks = 14 per compute unit exactly, and the workspace stays under 2 GiB
    assert lib.hmm_chunk_len(1, 1024, 100000, 15) == 448
    assert apply_blocks(1, 1024, 100000, 448) == 14 * CUS
    assert 0 < lib.hmm_workspace_bytes(engine.OP_POSTERIOR, 1, 1024, 100000, 15) < 2 << 30
    assert lib.hmm_chunk_len(1, 2048, 8200, 3) < MAX_T             # 544 blocks at 512: three per unit on 32 units


def test_rule_over_the_grid(lib):
    for k, b, L, q in GRID:
        assert lib.hmm_chunk_len(k, b, L, q) == rule(k, b, L), (k, b, L, q)


def test_forced_chunk_is_kept(lib):
    with engine.option(engine.OPT_CHUNK, 512):
        assert lib.hmm_chunk_len(1, 1024, 100000, 15) == 512
    with engine.option(engine.OPT_CHUNK, 64):
        assert lib.hmm_chunk_len(1, 1024, 100000, 15) == 64


# (k, b, L) -> chunk length at the commit before the rule, the same for q = 17, 29, 32, 48 and 64
SHAPES = [(1, 4, 128), (2, 3, 17), (1, 256, 10000), (1, 8, 100000), (1, 1, 1000000), (1, 1024, 100000),
          (1, 2048, 8200), (1, 4096, 9999)]
RECORDED = {"hmm_viterbi_scan_chunk_len": [16, 16, 320, 112, 144, 512, 512, 512],
            "hmm_loglik_grad_scan_chunk_len": [16, 16, 96, 272, 512, 512, 512, 512],
            "hmm_posterior_grad_scan_chunk_len": [16, 16, 96, 272, 512, 512, 512, 512]}
# hmm_posterior_grad_scan_chunk_len up to 16 states goes by its own rule (pc_chunk_len), q = 3 and 15
RECORDED_PG16 = [16, 17, 96, 272, 512, 512, 512, 512]
# hmm_viterbi_workspace_bytes holds the Viterbi plan's chunk length (q = 3 and 15)
RECORDED_VITERBI_WS = [57344, 24576, 63795456, 22379520, 16784384, 1089604096, 188476672, 442567936]


def test_other_plan_queries_are_unchanged(lib):
    for fn, want in RECORDED.items():
        for (k, b, L), t in zip(SHAPES, want):
            for q in (17, 29, 32, 48, 64):
                assert getattr(lib, fn)(k, b, L, q) == t, (fn, k, b, L, q)
    for (k, b, L), t, ws in zip(SHAPES, RECORDED_PG16, RECORDED_VITERBI_WS):
        for q in (3, 15):
            assert lib.hmm_posterior_grad_scan_chunk_len(k, b, L, q) == t, (k, b, L, q)
            assert lib.hmm_viterbi_workspace_bytes(k, b, L, q) == ws, (k, b, L, q)
            assert lib.hmm_chunk_len(k, b, L, q + 16) == 0
