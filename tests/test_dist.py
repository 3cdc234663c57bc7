"""Multi-rank tile-row sharding + gather over gloo, world_size 2/3.

Each rank renders only the tiles it owns (shard.tile_owner: round-robin tile
rows, the leftover rows cut into one run of tiles per rank) and TileGather
assembles the frame on rank 0; the result must equal a
single-rank render of the whole frame.  The CPU test renders the shards with
the oracle (this container has no GPU); the gpu-marked test renders them with
the HIP path, every rank on cuda:0, and gathers host tensors over gloo.
"""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, use_gpu, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from zenith_amd import scenes, shard
    s = scenes.soup_scene(31, 4000, 320, 256, 10.0, scenes.PROGRAM_BLINN_PHONG)
    if use_gpu:
        from zenith_amd import renderer, rhi
        dev = rhi.RenderDevice(0)
        color, _ = renderer.render_scene(dev, s, shard=(rank, world))
        dev.close()
    else:
        from oracle import oracle
        color, _ = oracle.render(s, shard=(rank, world))
    img = torch.from_numpy(np.ascontiguousarray(color).reshape(s.height, -1))
    g = shard.TileGather(s.width, s.height, 4, rank, world, torch.device("cpu"))
    g.gather(img)
    if rank == 0:
        np.save(out_path, img.numpy())
    dist.barrier()
    dist.destroy_process_group()


def _run(world, use_gpu, tmp_path):
    out = str(tmp_path / f"frame_{world}.npy")
    mp.spawn(_worker, args=(world, _free_port(), use_gpu, out), nprocs=world, join=True)
    return np.load(out)


def _full_frame():
    from oracle import oracle
    from zenith_amd import scenes
    s = scenes.soup_scene(31, 4000, 320, 256, 10.0, scenes.PROGRAM_BLINN_PHONG)
    color, _ = oracle.render(s)
    return color.reshape(s.height, -1)


@pytest.mark.parametrize("world", [2, 3])
def test_gloo_shard_gather_oracle(world, tmp_path):
    got = _run(world, False, tmp_path)
    assert np.array_equal(got, _full_frame())


@pytest.mark.parametrize("w,h", [(1920, 1080), (3840, 2160), (320, 256), (160, 120), (33, 1)])
def test_owned_tiles_partition(w, h):
    """Every pixel belongs to exactly one rank, and the tile counts differ by at
    most one between ranks (C2 at 8 ranks: 255 tiles each; round-robin rows alone
    gave 5 or 4 rows of 60)."""
    from zenith_amd import shard
    tx, ty = -(-w // 32), -(-h // 32)
    for world in (1, 2, 3, 5, 8, 32):
        masks = [shard.owned_mask(w, h, r, world) for r in range(world)]
        assert np.array_equal(sum(m.astype(np.int64) for m in masks), np.ones((h, w), np.int64))
        own = shard.tile_owner(tx, ty, world)
        counts = np.bincount(own.reshape(-1), minlength=world)
        assert counts.max() - counts.min() <= 1
        full = (ty // world) * world
        assert np.array_equal(own[:full], np.broadcast_to((np.arange(full) % world)[:, None], (full, tx)))
    assert list(np.bincount(shard.tile_owner(60, 34, 8).reshape(-1))) == [255] * 8
    assert list(np.bincount(shard.tile_owner(120, 68, 8).reshape(-1))) == [1020] * 8


@pytest.mark.gpu
def test_gloo_shard_gather_gpu(tmp_path):
    got = _run(2, True, tmp_path)
    assert np.array_equal(got, _full_frame())


# --------------------------------------- partitioned setup exchange protocol
def _spans(n, seed=5):
    """Per-primitive first/last tile row: culled (-1), single rows, spans up to 12 rows."""
    g = np.random.default_rng(seed)
    lo = g.integers(0, 34, n)
    hi = lo + np.minimum(g.geometric(0.5, n) - 1, 11)
    lo[g.random(n) < 0.1] = -1
    return lo, hi


def _expected(lo, hi, rank, world):
    from zenith_amd import shard
    own = shard.tile_owner(1, int(max(hi)) + 1, world)  # route_blocks' default target: one tile column
    return [p for p in range(len(lo)) if lo[p] >= 0 and rank in own[lo[p]:hi[p] + 1, 0]]


def _a2a_worker(rank, world, port, n, out_path):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from zenith_amd import shard
    lo, hi = _spans(n)
    send = shard.route_blocks(lo, hi, rank, world).reshape(-1)
    recv = torch.empty_like(send)
    dist.all_to_all_single(recv, send)  # RcclExchange's call, on host tensors
    got, over = shard.received_primitives(recv, n, world)
    ok = sorted(got) == _expected(lo, hi, rank, world) and not over
    np.save(f"{out_path}.{rank}.npy", np.array([ok]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,n", [(2, 9000), (3, 5000)])
def test_gloo_partitioned_exchange(world, n, tmp_path):
    """k_route's block layout (host model) through an all_to_all_single over gloo:
    every rank receives exactly the primitives touching its tile rows (several
    route chunks per rank at n=9000, G=2)."""
    out = str(tmp_path / "a2a")
    mp.spawn(_a2a_worker, args=(world, _free_port(), n, out), nprocs=world, join=True)
    for r in range(world):
        assert bool(np.load(f"{out}.{r}.npy")[0]), f"rank {r}"


def test_route_blocks_model():
    """Single-process check of the block model at G=8 (ranks with empty ranges)."""
    from zenith_amd import shard
    n, world = 20000, 8
    lo, hi = _spans(n, seed=9)
    sends = [shard.route_blocks(lo, hi, r, world) for r in range(world)]
    for d in range(world):
        recv = torch.stack([sends[s][d] for s in range(world)])
        got, over = shard.received_primitives(recv, n, world)
        assert sorted(got) == _expected(lo, hi, d, world) and not over


def test_route_blocks_overflow():
    """A block capacity below a destination's share: the block keeps `cap`
    entries, its header says total > count, and the receiver sees the overflow
    (the device then sets up the whole draw on that rank)."""
    from zenith_amd import shard
    n, world, cap = 6000, 4, 100
    lo, hi = _spans(n, seed=3)
    sends = [shard.route_blocks(lo, hi, r, world, cap=cap) for r in range(world)]
    for d in range(world):
        recv = torch.stack([sends[s][d] for s in range(world)])
        got, over = shard.received_primitives(recv, n, world, cap=cap)
        assert over and len(got) == world * cap
        assert set(got) <= set(_expected(lo, hi, d, world))


def test_route_model_matches_device_constants():
    """The host route model uses the kernels' chunk size, entry and header sizes
    (zr_internal.h) and the plan's default capacity (zr_plan.cpp)."""
    import re
    from zenith_amd import shard
    src = open(os.path.join(ROOT, "zenith_amd", "csrc", "zr_internal.h")).read()
    assert int(re.search(r"#define ZR_ROUTE_CHUNK (\d+)", src).group(1)) == shard.ROUTE_CHUNK
    assert 'sizeof(RouteEntry) == 48' in src and 'sizeof(RouteHeader) == 16' in src
    rt = open(os.path.join(ROOT, "zenith_amd", "csrc", "zr_plan.cpp")).read()
    assert "std::min<uint64_t>(span, (2 * span + G - 1) / G + 4096)" in rt and "if (G <= 2) return span;" in rt
    # 1M primitives over 8 ranks: span rounds ceil(N / G) up to whole chunks
    chunks, span, cap, bb = shard.route_geometry(1_000_000, 8)
    assert span == 125_440 and chunks == span // shard.ROUTE_CHUNK
    assert cap == 2 * span // 8 + 4096 and bb == 16 + 48 * cap
    assert shard.route_range(1_000_000, 7, 8) == (7 * 125_440, 1_000_000)
