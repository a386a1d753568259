"""ured_copy_batch (csrc/copy.hip): the HIP-graph steps' batched refresh of their static inputs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_copy_batch_units_and_sizes(dev):
    from ured_hip.ops import copy_batch
    g = torch.Generator(device=dev).manual_seed(0)
    base = torch.randint(0, 255, (4099,), device=dev, dtype=torch.uint8, generator=g)
    srcs = [torch.randn(16, 2048, 3, device=dev, generator=g),               # 16-B units
            torch.randint(-5, 5, (16, 2048), device=dev, generator=g),       # int64
            torch.randn(7, device=dev, generator=g),                         # 28 B: 4-B units
            base[1:4098],                                                    # odd offset and size: 1-B units
            torch.empty(0, device=dev)]                                      # empty: skipped
    srcs += [torch.randn(5, 3, device=dev, generator=g) for _ in range(14)]  # 19 items: two launches
    dsts = [torch.full_like(s, 7) for s in srcs]
    copy_batch(list(zip(dsts, srcs)))
    for d, s in zip(dsts, srcs):
        assert torch.equal(d, s)
    with pytest.raises(ValueError):
        copy_batch([(torch.empty(3, device=dev), torch.empty(4, device=dev))])


SENTINEL, GUARD = 0xA5, 64


def _arena_copy(dev, items, seed, max_launch_items=None):
    """copy_batch over items = [(bytes, source offset, destination offset)] laid out in two byte
    arenas: item i occupies [start_i + off, start_i + off + bytes) with start_i a multiple of 64, so the
    offsets (0..15) are the addresses' alignment, and at least GUARD sentinel bytes separate
    neighbouring destinations and the arena's ends. The whole destination arena is compared with the
    expected bytes: every destination equals its source and no byte outside one has changed."""
    from ured_hip.ops import COPY_MAX, copy_batch
    assert len(items) <= (max_launch_items or COPY_MAX)
    starts, pos = [], GUARD
    for size, so, do in items:
        assert 0 <= so < 16 and 0 <= do < 16
        starts.append(pos)
        pos = -(-(pos + 16 + size + GUARD) // 64) * 64
    total = pos + GUARD
    rng = np.random.Generator(np.random.PCG64(seed))
    src_h = rng.integers(0, 256, size=total, dtype=np.uint8)
    exp_h = np.full(total, SENTINEL, np.uint8)
    src, dst = torch.from_numpy(src_h).to(dev), torch.full((total,), SENTINEL, dtype=torch.uint8, device=dev)
    assert src.data_ptr() % 64 == 0 and dst.data_ptr() % 64 == 0
    pairs = []
    for (size, so, do), st in zip(items, starts):
        pairs.append((dst[st + do:st + do + size], src[st + so:st + so + size]))
        exp_h[st + do:st + do + size] = src_h[st + so:st + so + size]
    copy_batch(pairs)
    got = dst.cpu().numpy()
    bad = np.flatnonzero(got != exp_h)
    assert bad.size == 0, f"{bad.size} wrong bytes, first at {bad[0]} (item starts {starts}, items {items})"


def test_copy_batch_guard_bands_and_alignments(dev):
    """Each unit width reached from each side: 16-B units (aligned pointers and size), 4-B units forced
    by the destination (source 16-B aligned, destination 4 bytes on), by the size (both aligned, 20
    bytes) and by both; 1-B units from an odd offset with a size that is a multiple of 16, from an odd
    size, and one byte; an empty item between them."""
    _arena_copy(dev, [(4096, 0, 0), (4096, 0, 4), (20, 0, 0), (4100, 8, 12), (4096, 3, 3), (1024, 0, 5),
                      (0, 0, 0), (37, 0, 0), (1, 15, 0), (16, 0, 0), (48, 4, 0)], 1)


def test_copy_batch_grid_stride_crosses_items(dev):
    """600000 16-B units in the first item: more than the 2048 x 256 threads of the largest grid, so the
    threads make a second trip, in which the high ones run past the large item into the small items of
    each unit width that follow it."""
    first = 600000 * 16
    assert first // 16 > 2048 * 256
    _arena_copy(dev, [(first, 0, 0), (20, 0, 0), (4096, 0, 0), (333, 1, 2), (16, 0, 0), (4, 4, 8), (70000, 0, 4),
                      (1, 0, 0), (65536, 0, 0)], 2)


def test_copy_batch_max_items_in_one_call(dev):
    """Exactly URED_COPY_MAX non-empty items: one launch, the last slot of the item table in use."""
    from ured_hip.ops import COPY_MAX
    assert COPY_MAX == 16
    _arena_copy(dev, [(16 * (i + 1) + (i % 3) * 4, (5 * i) % 16 if i % 2 else 0, (3 * i) % 16 if i % 4 == 3 else 0)
                      for i in range(COPY_MAX)], 3, max_launch_items=COPY_MAX)


def _sweep_batches():
    rng = np.random.Generator(np.random.PCG64(424242))
    out = []
    for _ in range(24):
        k = int(rng.integers(1, 17))
        sizes = rng.integers(0, 70001, size=k)
        sizes[rng.random(k) < 0.3] //= 16                       # small items too
        sizes[rng.random(k) < 0.3] &= ~15                       # and sizes that are multiples of 16
        al = rng.random(k) < 0.4                                # 16-B aligned on both sides
        so, do = np.where(al, 0, rng.integers(0, 16, size=k)), np.where(al, 0, rng.integers(0, 16, size=k))
        out.append([(int(s), int(a), int(b)) for s, a, b in zip(sizes, so, do)])
    return out


def test_copy_batch_seeded_sweep(dev):
    """24 batches of 1-16 items, 0-70000 bytes each, source and destination offsets 0-15, every
    destination between guard bands."""
    batches = _sweep_batches()
    units = set()
    for i, items in enumerate(batches):
        units |= {16 if (s | a | b) % 16 == 0 else 4 if (s | a | b) % 4 == 0 else 1 for s, a, b in items if s}
        _arena_copy(dev, items, 100 + i)
    assert units == {1, 4, 16}, "the sweep must reach every unit width"


def test_refresh_static_unique_rows(dev):
    import numpy as np
    from ured_hip.ops import PartBounds, UniqueRows, refresh_static
    lab = np.array([[3, -1, 5, 3], [-1, -1, 2, 7]])
    lab2 = np.array([[4, -1, 1, 4], [-1, -1, 0, 6]])
    static = {"x": torch.zeros(2, 8, 3, device=dev), "src_unique": UniqueRows(lab, 10, dev, bucket=8),
              "part_bounds": PartBounds(np.zeros((2, 8)))}
    x = torch.randn(2, 8, 3, device=dev)
    batch = {"x": x, "src_unique": UniqueRows(lab2, 10, dev, bucket=8), "part_bounds": PartBounds(np.zeros((2, 8)))}
    refresh_static(static, batch)
    assert torch.equal(static["x"], x)
    for f in UniqueRows.FIELDS:
        assert torch.equal(getattr(static["src_unique"], f), getattr(batch["src_unique"], f)), f
