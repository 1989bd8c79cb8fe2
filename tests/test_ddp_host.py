"""CPU tests of data-parallel training's host side: the gradient bucket's layout (optim.bucket_layout), the sharded
BatchIterator, parallel.all_reduce_sum under gloo, the ``--gpus`` flag of MODE=train, and the declaration and binding of
fv_grad_bucket_pack."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from fastvocoder_amd import _native, data, optim, parallel
from fastvocoder_amd.bin import train as train_cli

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOP = 12


# ---- the bucket ------------------------------------------------------------------------------------------------------

def _params(sizes, frozen=()):
    return [torch.nn.Parameter(torch.zeros(n), requires_grad=k not in frozen) for k, n in enumerate(sizes)]


def test_bucket_offsets_are_16_byte_aligned_and_spans_do_not_overlap():
    sizes = [1, 7, 4096, 4097, 4099]
    offsets, total = optim.bucket_layout(_params(sizes))
    assert offsets == [0, 4, 12, 4108, 8208] and total == 4 + 8 + 4096 + 4100 + 4100
    assert all(off % 4 == 0 for off in offsets) and total % 4 == 0
    for (a, n), b in zip(zip(offsets, sizes), offsets[1:] + [total]):
        assert a + n <= b and b - a == (n + 3) // 4 * 4          # a span is the size rounded up to 4 floats


@pytest.mark.parametrize("n", [1, 7, 4096, 4097, 4099])
def test_bucket_total_of_one_tensor(n):
    assert optim.bucket_layout(_params([n])) == ([0], (n + 3) // 4 * 4)


def test_bucket_leaves_out_parameters_that_do_not_require_grad():
    sizes = [5, 9, 3, 16]
    offsets, total = optim.bucket_layout(_params(sizes, frozen=(1,)))
    assert offsets == [0, 8, 12] and total == 28
    assert optim.bucket_layout(_params(sizes, frozen=(0, 1, 2, 3))) == ([], 0)
    assert optim.bucket_layout(p for p in _params([2, 3])) == ([0, 4], 8)      # any iterable, a shape of any rank
    assert optim.bucket_layout([torch.nn.Parameter(torch.zeros(3, 5, 2))]) == ([0], 32)


def test_the_table_carries_the_source_pointers_behind_the_chunks():
    rows = [(16, 32, 48, 64, 5000, 0.5, 1.0), (80, 96, 112, 128, 3, 0.5, 1.0)]
    plain, first = optim.adam_table(rows)
    with_src, first2 = optim.adam_table(rows, [4096, 0])
    assert list(first) == list(first2) == [0, 2, 3]
    assert plain.size == 2 * _native.ADAM_ROW_BYTES + 3 * _native.ADAM_CHUNK_BYTES
    assert np.array_equal(with_src[:plain.size], plain)
    assert with_src[plain.size:].view("<u8").tolist() == [4096, 0] and plain.size % 8 == 0
    with pytest.raises(ValueError):
        optim.adam_table(rows, [1])


# ---- the sharded batches ---------------------------------------------------------------------------------------------

def _buffer(frames):
    rs = np.random.RandomState(4)
    return [{"mel": torch.from_numpy(rs.rand(f, 80).astype(np.float32)),
             "wav": torch.from_numpy(rs.rand(f * HOP).astype(np.float32))} for f in frames]


@pytest.mark.parametrize("world", [2, 3])
def test_rank_batches_concatenate_to_the_single_process_batch(world, capsys):
    frames = [9, 30, 4, 12, 17, 8, 3, 25, 11, 16, 14, 40, 10]          # 13 utterances, 3 too short for 8 frames + 1
    per_rank, fixed = 2, 8
    buffer = _buffer(frames)
    whole = data.BatchIterator(buffer, per_rank * world, fixed, HOP, seed=5)
    ranks = [data.BatchIterator(buffer, per_rank, fixed, HOP, seed=5, rank=r, world_size=world) for r in range(world)]
    assert whole.skipped == 3 and all(it.skipped == 3 for it in ranks)
    assert len(whole) == 10 // (per_rank * world) and all(len(it) == len(whole) for it in ranks)
    assert len(whole) >= 1
    for _ in range(2):                                   # two epochs: the streams stay in step
        got = [list(it.epoch()) for it in ranks]
        want = list(whole.epoch())
        assert all(len(g) == len(want) for g in got)
        for b, (mel, wav) in enumerate(want):
            assert torch.equal(torch.cat([g[b][0] for g in got]), mel)
            assert torch.equal(torch.cat([g[b][1] for g in got]), wav)
            assert all(g[b][0].shape == (per_rank, fixed, 80) for g in got)
    capsys.readouterr()


def test_a_rank_outside_the_world_is_refused():
    for rank, world in ((2, 2), (-1, 2), (0, 0)):
        with pytest.raises(ValueError, match="rank"):
            data.BatchIterator(_buffer([20]), 1, 8, HOP, rank=rank, world_size=world)
    it = data.BatchIterator(_buffer([20, 20]), 1, 8, HOP)
    assert (it.rank, it.world_size, len(it)) == (0, 1, 2)


# ---- the collective --------------------------------------------------------------------------------------------------

def _reduce_worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        t = (torch.arange(1001, dtype=torch.float32) * (rank + 1) + rank).reshape(7, 143)
        out = parallel.all_reduce_sum(t, dist.group.WORLD)
        assert out is t                                           # in place
        want = (torch.arange(1001, dtype=torch.float32) * 3 + 1).reshape(7, 143)
        assert torch.equal(t, want)                               # integers stored as floats: the sum is exact
        d = torch.tensor([2.0 ** 40 + rank], dtype=torch.float64)
        assert float(parallel.all_reduce_sum(d)) == 2.0 ** 41 + 1           # group None: the default group
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_all_reduce_sum_is_exact_under_gloo():
    mp.spawn(_reduce_worker, args=(2, 29561), nprocs=2, join=True)


# ---- the command line ------------------------------------------------------------------------------------------------

def test_gpus_is_absent_unless_given_and_check_args_takes_it():
    parser = train_cli.build_parser()
    assert "gpus" not in vars(parser.parse_args([]))
    base = ["--model_name", "hifigan", "--config", "c.yaml"]
    args = train_cli.check_args(parser.parse_args(base + ["--gpus", "2"]))
    assert args.gpus == 2
    assert "gpus" not in vars(train_cli.check_args(parser.parse_args(base)))
    with pytest.raises(SystemExit) as e:
        train_cli.check_args(parser.parse_args(base + ["--gpus", "0"]))
    assert "--gpus" in str(e.value)


def test_the_launch_line_and_the_refusal():
    argv = train_cli.self_launch_argv(4, ["--model_name", "hifigan", "--gpus", "4"], 29512)
    assert argv[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert argv[argv.index("--nproc-per-node") + 1] == "4" and argv[argv.index("--master-port") + 1] == "29512"
    assert argv[-6:] == ["-m", "fastvocoder_amd.bin.launcher", "--model_name", "hifigan", "--gpus", "4"]
    assert train_cli.visible_devices_error(2, 2) is None and train_cli.visible_devices_error(1, 8) is None
    err = train_cli.visible_devices_error(3, 1)
    assert "--gpus 3 needs 3 visible devices, this node shows 1" in err and err.count("\n") == 0


# ---- the ABI ---------------------------------------------------------------------------------------------------------

def test_the_pack_entry_is_declared_and_bound_under_abi_18():
    header = open(os.path.join(ROOT, "include", "fastvocoder_hip.h")).read()
    assert re.search(r"^#define FV_ABI_VERSION 18\b", header, flags=re.M) and _native.ABI_VERSION == 18
    decl = re.search(r"^int fv_grad_bucket_pack\(([^;]*)\);", header, flags=re.M | re.S)
    assert decl, "fv_grad_bucket_pack is not declared in include/fastvocoder_hip.h"
    args = " ".join(decl.group(1).split())
    assert args == ("const fv_adam_tensor* tensors, const fv_adam_chunk* chunks, int n_tensors, int64_t n_chunks, "
                    "const float* const* src, float scale, void* stream")
    vp = ctypes.c_void_p
    assert list(_native.lib().fv_grad_bucket_pack.argtypes) == [vp, vp, ctypes.c_int, ctypes.c_int64, vp, ctypes.c_float, vp]
    assert callable(_native.grad_bucket_pack)
    assert "fv_grad_bucket_pack" in open(os.path.join(ROOT, "fastvocoder_amd", "csrc", "optim.hip")).read()
