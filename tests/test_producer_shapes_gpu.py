"""The actuator, normaliser and event kernels against their restatements in oracle/ run in float64 on the same fp32
inputs, beyond the one fixture shape each is pinned at in test_producers.py: odd sample counts, every network shape the four LSTM kernels
take, history / delay edges, normaliser statistics at large counts and means, event masks at env counts that are not multiples of a block.
Floats within the tests/_util.py tolerance rules; levels, ids, masks, histories and delay rings bit for bit.  Cases: tests/_producer_cases.py."""
import pytest
import torch

from _producer_cases import (delayed_case, events_case, lstm_case, lstm_in_child, mlp_case, normalizer_case, pd_case)

pytestmark = pytest.mark.gpu

# (N, J) with N * J in {1, 31, 127, 129, 4096 * 12, 4097 * 12, 100 003}
SHAPES = [(1, 1), (31, 1), (127, 1), (43, 3), (4096, 12), (4097, 12), (100003, 1)]

# the ANYdrive shapes the fast kernels take: hidden 8, 1-4 layers, a head of 8 -> 1 or 8 -> 16 | 32 -> 1, every activation
FAST = [dict(N=N, J=J, H=8, L=L, head=head, act=act, seed=100 + k, steps=8)
        for k, ((N, J), L, head, act) in enumerate(zip(SHAPES, (1, 2, 3, 4, 2, 1, 4), ([], [16], [32], [16], [32], [16], [32]),
                                                          ("softsign", "softsign", "tanh", "relu", "elu", "identity", "softsign")))]

# what only the generic LDS kernel takes: hidden != 8, more than 4 layers, a head width other than 16 / 32, two hidden head layers,
# state tensors off a 16-byte boundary
GENERIC = [
    dict(N=1, J=1, H=1, L=1, head=[], act="identity", seed=200),
    dict(N=31, J=1, H=5, L=5, head=[24], act="softsign", seed=201),
    dict(N=43, J=3, H=16, L=5, head=[16], act="tanh", seed=202),
    dict(N=127, J=1, H=32, L=3, head=[32], act="relu", seed=203),
    dict(N=4097, J=12, H=16, L=2, head=[24, 8], act="elu", seed=204),
    dict(N=100003, J=1, H=5, L=2, head=[24], act="identity", seed=205),
    dict(N=4096, J=12, H=8, L=2, head=[8], act="softsign", seed=206),
    dict(N=129, J=1, H=8, L=5, head=[16], act="tanh", seed=207),
    dict(N=4097, J=12, H=8, L=2, head=[16], act="elu", seed=208, unaligned=True),
    dict(N=31, J=1, H=8, L=1, head=[], act="relu", seed=209, unaligned=True),
]


def test_lstm_matrix_core_kernel_at_every_fast_shape():
    for kw in FAST:
        lstm_case(**kw)


def test_lstm_generic_kernel_shapes_and_unaligned_state():
    for kw in GENERIC:
        lstm_case(**kw)


@pytest.mark.parametrize("kernel", ["l", "r"])
def test_lstm_lanes_and_register_kernels_in_a_child_process(kernel):
    """``IMX_LSTM_KERNEL`` is read once per process: each variant runs the fast shapes in a fresh interpreter of its own."""
    code, out = lstm_in_child(kernel, FAST)
    assert code == 0, f"IMX_LSTM_KERNEL={kernel} child exited with {code}:\n{out[-3000:]}"
    assert out.count(f"IMX_LSTM_KERNEL={kernel}: lstm ") == len(FAST), out[-3000:]


MLP = [([0], "pos_vel", [16]), ([0, 2, 5], "vel_pos", [32, 8]), ([3, 0], "pos_vel", [24]), ([1, 1], "vel_pos", [16, 16, 16]),
       ([0], "vel_pos", [8]), ([0, 2, 5], "pos_vel", [24]), ([3, 0], "vel_pos", [32]), ([1, 1], "pos_vel", [16])]


def test_mlp_actuator_net_histories_orders_and_activations():
    acts = ("softsign", "tanh", "relu", "elu", "identity")
    for k, (idx, order, widths) in enumerate(MLP):
        N, J = SHAPES[k % len(SHAPES)] if k < 7 else (65, 12)
        mlp_case(N, J, idx, order, acts[k % len(acts)], widths, seed=300 + k, scales=(1.7, 0.35, 3.0) if k % 2 else (0.5, 2.0, 12.0))


@pytest.mark.parametrize("max_delay", [0, 1, 4, 37])
def test_delayed_and_remotized_pd_ring_and_lookup_edges(max_delay):
    min_delay = 0 if max_delay < 4 else 2
    delayed_case(63, 12, min_delay, max_delay, None, seed=400 + max_delay)
    for K in (1, 2, 9):
        delayed_case(65, 3, min_delay, max_delay, K, seed=410 + 7 * max_delay + K)
    if max_delay == 4:
        delayed_case(4097, 12, 0, 4, 9, seed=450)


def test_pd_and_dc_motor_at_clip_corners():
    for k, (N, J) in enumerate(SHAPES):
        pd_case(N, J, seed=500 + k, dc=True)
    pd_case(4097, 12, seed=520, dc=False)


@pytest.mark.parametrize("D,batches", [(1, (1, 2, 63, 4096, 100003)), (64, (4096, 63, 1, 2)), (65, (2, 100003, 63)),
                                       (235, (4096, 4096, 1, 63)), (310, (63, 100003, 2))])
def test_normalizer_statistics_against_fp64(D, batches):
    normalizer_case(D, batches, seed=600 + D)


def test_normalizer_count_stays_exact_past_two_to_the_24():
    """~170 batches of 100 003 rows: the running count passes 2^24, where an fp32 count stops being exact for an odd batch size."""
    from isaaclab_amd.rsl_rl.normalizer import EmpiricalNormalization
    from oracle.rsl_rl_oracle import EmpiricalNormalizationOracle

    N, calls = 100003, 170
    g = torch.Generator().manual_seed(7)
    x = torch.randn(N, 1, generator=g) * 0.5 + 0.25
    xd = x.cuda()
    norm = EmpiricalNormalization([1]).cuda()
    orc = EmpiricalNormalizationOracle(1)
    orc.mean, orc.var, orc.std = (t.double() for t in (orc.mean, orc.var, orc.std))
    for _ in range(calls):
        norm(xd)
        orc.forward(x.double(), training=True)
    assert orc.count == N * calls > 2 ** 24
    assert norm.count == orc.count, f"count {int(norm.count)} vs {orc.count}"
    assert norm.count.dtype == torch.int64
    assert abs(float(norm._mean) - float(orc.mean)) <= 1e-5 and abs(float(norm._var) - float(orc.var)) <= 1e-5


@pytest.mark.parametrize("N", [1, 63, 65, 4097, 100003])
def test_events_against_fp64_at_ragged_env_counts(N):
    NB = 17
    body_ids = {1: [4], 63: None, 65: [0, 3, 16], 4097: [16], 100003: [2, 5, 7, 11]}[N]
    R, C = {1: (1, 1), 63: (10, 1), 65: (1, 20), 4097: (10, 20), 100003: (6, 4)}[N]
    events_case(N, 12, NB, R, C, seed=700 + N, body_ids=body_ids, degenerate=N in (63, 4097))


def test_mean_levels_at_100k_envs():
    from isaaclab_amd.events import TerrainCurriculum

    N, R, C = 100003, 10, 20
    g = torch.Generator().manual_seed(8)
    levels = torch.randint(0, R, (N,), generator=g)
    types = torch.randint(0, C, (N,), generator=g)
    grid = torch.randn(R, C, 3, generator=g)
    lv = levels.cuda()
    cur = TerrainCurriculum(grid.cuda(), lv, types.cuda(), grid[levels, types].cuda(), 8.0, 20.0)
    mask = torch.zeros(N, dtype=torch.uint8, device="cuda")  # nobody moves: the mean of the levels as they are
    mean = cur.update(mask, grid[levels, types].cuda(), torch.zeros(N, 3, device="cuda"))
    assert torch.equal(lv.cpu(), levels)
    ref = levels.double().mean()
    assert abs(float(mean) - float(ref)) <= 1e-5 * max(1.0, float(ref)), (float(mean), float(ref))
