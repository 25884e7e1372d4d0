"""tests/_blob.py on blobs synthesised from _blob_layout, without a GPU: parse() accounts for every byte, canonical() is
idempotent and blind to the done list's order, permute_done_list() touches nothing but the list, and a done counter past the
batch size is refused."""
import numpy as np
import pytest

from _blob import HEADER_BYTES, _blob_layout, _walk, canonical, header, parse, permute_done_list

SHAPES = {
    "simple_game": (dict(simple_game=True), 2 * 16),
    "simple_race_minstd": (dict(simple_race=True, minstd=True), 16),
    "xworld_full": (dict(cells=49), 2 * 3 * 84 * 84),
    "xworld_ego": (dict(cells=49, ego=True), None),
    "xworld_exclusive_minstd": (dict(cells=49, groups=2, exclusive=True, minstd=True), 84 * 84),
    "xworld_curriculum": (dict(cells=64, curriculum=True), None),
}
N = 300


def _synth(shape, frames, n=N, list_valid=1, done=(), seed=1):
    """a version-4 blob with random bytes in every array, `done` as the first entries of its done list"""
    rng = np.random.default_rng(seed)
    lengths = _blob_layout(n, frames, **shape)
    head = np.zeros(HEADER_BYTES, np.uint8)
    head[:8] = np.frombuffer(b"XWBSTATE", np.uint8)
    head[8:40].view("<u4")[:] = [4, 2 if shape.get("cells") else 0, n, int(frames is not None), len(lengths), 41, 0, list_valid]
    head[40:56].view("<u8")[:] = [frames or 0, 0x1234567890abcdef]
    parts = [head]
    for length in lengths:
        parts += [np.array([length], "<u8").view(np.uint8), rng.integers(0, 256, length, dtype=np.uint8)]
    blob = np.concatenate(parts)
    if shape.get("cells"):
        p = parse(blob, **shape)
        p["done_count"][0] = len(done)
        p["done_list"][:len(done)] = done
    return blob


@pytest.mark.parametrize("case", sorted(SHAPES))
def test_parse_consumes_every_byte(case):
    shape, frames = SHAPES[case]
    blob = _synth(shape, frames)
    p = parse(blob, **shape)
    h = p.pop("header")
    assert h == header(blob) and h["num_envs"] == N and h["version"] == 4 and h["policy_step"] == 41
    n_arrays, lengths = _walk(blob)
    assert len(p) == n_arrays == len(lengths)                           # every array has a name of its own
    assert sum(v.nbytes for v in p.values()) + 8 * n_arrays + HEADER_BYTES == blob.size
    covered = np.zeros(blob.size, np.uint8)
    covered[:HEADER_BYTES] = 1
    base = blob.__array_interface__["data"][0]
    for (name, v), length in zip(p.items(), lengths):
        at = v.__array_interface__["data"][0] - base
        assert v.nbytes == length and int.from_bytes(blob[at - 8:at].tobytes(), "little") == length, name
        covered[at - 8:at + length] += 1
        if v.ndim == 2:
            assert v.shape[0] == N, name
    assert (covered == 1).all()                                         # each byte once: no overlap, no gap
    assert ("done_list" in p) == bool(shape.get("cells")) and ("obs" in p) == (frames is not None)
    if "obs" in p:
        assert p["obs"].shape == (N, frames)
    with pytest.raises(AssertionError):                                 # a shape that names other arrays does not fit
        parse(blob, **dict(shape, minstd=not shape.get("minstd", False)))
    with pytest.raises(AssertionError):
        parse(blob[:-1], **shape)


@pytest.mark.parametrize("case", ["xworld_full", "xworld_exclusive_minstd", "xworld_curriculum"])
def test_canonical_and_permute(case):
    shape, frames = SHAPES[case]
    done = [299, 3, 64, 65, 0, 255, 256, 128, 17]
    blob = _synth(shape, frames, done=done)
    keep = blob.copy()
    c = canonical(blob, **shape)
    assert np.array_equal(blob, keep)                                   # (the argument is left alone)
    assert np.array_equal(canonical(c, **shape), c)                     # idempotent
    pc = parse(c, **shape)
    assert pc["done_list"][:len(done)].tolist() == sorted(done) and not pc["done_list"][len(done):].any()
    rng = np.random.default_rng(7)
    for perm in (range(len(done))[::-1], rng.permutation(len(done)), range(len(done))):
        q = permute_done_list(blob, perm, **shape)
        assert np.array_equal(blob, keep)
        pq, pb = parse(q, **shape), parse(blob, **shape)
        assert pq["done_list"][:len(done)].tolist() == [done[i] for i in perm]
        assert np.array_equal(pq["done_list"][len(done):], pb["done_list"][len(done):])
        for name in pb:                                                 # nothing but the list changes
            if name not in ("done_list", "header"):
                assert pq[name].tobytes() == pb[name].tobytes(), name      # (bytes: random floats hold NaNs)
        assert pq["header"] == pb["header"] and q.size == blob.size
        differs = np.nonzero(q != blob)[0]
        lo = pb["done_list"].__array_interface__["data"][0] - blob.__array_interface__["data"][0]
        assert differs.size == 0 or (differs.min() >= lo and differs.max() < lo + 4 * len(done))
        assert np.array_equal(canonical(q, **shape), c)                 # invariant under the order
    other = _synth(shape, frames, done=done[:-1] + [18])                # another SET of envs is another canonical blob
    assert not np.array_equal(canonical(other, **shape), c)
    with pytest.raises(AssertionError):
        permute_done_list(blob, [0] * len(done), **shape)


def test_canonical_without_a_valid_list():
    shape, frames = SHAPES["xworld_full"]
    blob = _synth(shape, frames, list_valid=2, done=[5, 4, 3])          # (bit 1 alone: step_autoreset's codes, no list)
    c = canonical(blob, **shape)
    assert not parse(c, **shape)["done_list"].any() and parse(c, **shape)["done_count"][0] == 3
    assert np.array_equal(canonical(c, **shape), c)
    with pytest.raises(AssertionError):
        permute_done_list(blob, [2, 1, 0], **shape)
    sg, f = SHAPES["simple_game"]
    blob = _synth(sg, f)
    assert np.array_equal(canonical(blob, **sg), blob)                  # the simple games have no list
    with pytest.raises(AssertionError):
        permute_done_list(blob, [], **sg)


@pytest.mark.parametrize("count", [N + 1, -1, 1 << 30])
def test_done_count_past_the_batch_is_rejected(count):
    shape, frames = SHAPES["xworld_ego"]
    blob = _synth(shape, frames, done=[1, 2])
    parse(blob, **shape)["done_count"][0] = count
    with pytest.raises(AssertionError, match="done_count"):
        canonical(blob, **shape)
    with pytest.raises(AssertionError, match="done_count"):
        permute_done_list(blob, [1, 0], **shape)
    parse(blob, **shape)["done_count"][0] = N                          # exactly n is a full list
    parse(blob, **shape)["done_list"][:] = np.arange(N)[::-1]
    assert parse(canonical(blob, **shape), **shape)["done_list"].tolist() == list(range(N))
