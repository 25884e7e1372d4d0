"""The version-4 state blob of xwb_save_state, written out on the test side and not taken from the library: a header of 56
bytes, then a uint64 length in front of each array.  parse() names the arrays, canonical() removes the one thing about a blob
that is allowed to differ between two runs of the same rollout -- the order in which the wavefronts of a step appended the
finished envs to the done list -- and permute_done_list() makes a blob that differs in nothing else."""
import numpy as np

XW_USAGE_BYTES, XW_MAX_GOALS = 32, 16
HEADER_BYTES = 56
# the header's uint32 fields after the 8-byte magic, then two uint64: obs_bytes_per_env, cfg_hash
HEADER_U32 = ("version", "game", "num_envs", "include_obs", "n_arrays", "policy_step", "count_sel", "list_valid")


def _blob_layout(n, frames, cells=0, simple_game=False, simple_race=False, minstd=False, groups=1, exclusive=False, ego=False,
                 curriculum=False):
    """The lengths of a version-4 blob's arrays, in order (n envs, `frames` bytes of frames per env or None, cells = max_dim^2)."""
    a = [4 * n, 4 * n, 4 * n, 4 * n, n, n, 4, 4 * ((n + 255) // 256)]        # actions, num_steps, episode, reward, done, success, errors, reset counts
    if simple_game:
        a += [4 * n, n]
    if simple_race:
        a += [4 * n, 4 * n, 4 * n]
    if minstd:
        a += [4 * n]
    if cells:
        a += [2 * n * cells, 4 * n, 4 * n, 4 * n]                            # grid, agent, task steps, task state
        if groups == 2:
            a += [4 * n, 4 * n]
            if exclusive:
                a += [n]
        a += [4 * n, 4, n, 320, XW_MAX_GOALS * n, 4 * n, n, 4 * n]           # done list, its counter, fresh, perf, goal cells, cand2d, heading, names
        if ego:
            a += [XW_MAX_GOALS * 6 * 8 * n]                                  # goal warps: 768 n
        if curriculum:
            a += [n, 4 * n, 9 * n * XW_USAGE_BYTES]
    if frames is not None:
        a += [n * frames]
    return a


def _blob_names(frames, cells=0, simple_game=False, simple_race=False, minstd=False, groups=1, exclusive=False, ego=False,
                curriculum=False):
    """(name, element type) of the arrays _blob_layout counts, in the same order: the names of its comments"""
    a = [("actions", "<i4"), ("num_steps", "<i4"), ("episode", "<u4"), ("reward", "<f4"), ("done", "u1"), ("success", "u1"),
         ("errors", "<i4"), ("reset_counts", "<i4")]
    if simple_game:
        a += [("pos", "<i4"), ("flags", "u1")]
    if simple_race:
        a += [("x", "<f4"), ("y", "<f4"), ("angle", "<f4")]
    if minstd:
        a += [("minstd", "<u4")]
    if cells:
        a += [("grid", "<u2"), ("agent", "<u4"), ("task_steps", "<i4"), ("task_state", "<u4")]
        if groups == 2:
            a += [("task_steps2", "<i4"), ("task_state2", "<u4")]
            if exclusive:
                a += [("grp_order", "u1")]
        a += [("done_list", "<i4"), ("done_count", "<i4"), ("fresh", "u1"), ("perf", "<i8"), ("goal_cells", "u1"), ("cand2d", "<u4"),
              ("heading", "u1"), ("names", "<u4")]
        if ego:
            a += [("goal_warps", "<f8")]
        if curriculum:
            a += [("cur_level", "u1"), ("cur_counter", "<i4"), ("cur_usage", "u1")]
    if frames is not None:
        a += [("obs", "u1")]
    return a


def _walk(blob):
    """(n_arrays of the 56-byte header, the uint64 length in front of each array), the blob consumed to its last byte"""
    raw = blob.tobytes()
    assert raw[:8] == b"XWBSTATE" and int.from_bytes(raw[8:12], "little") == 4
    n_arrays, at, lengths = int.from_bytes(raw[24:28], "little"), 56, []
    while at < len(raw):
        lengths.append(int.from_bytes(raw[at:at + 8], "little"))
        at += 8 + lengths[-1]
    assert at == len(raw)
    return n_arrays, lengths


def header(blob):
    """the header's fields as a dict of ints"""
    blob = np.asarray(blob, np.uint8)
    assert blob.size >= HEADER_BYTES and blob[:8].tobytes() == b"XWBSTATE"
    h = dict(zip(HEADER_U32, (int(v) for v in blob[8:40].view("<u4"))))
    h["obs_bytes_per_env"], h["cfg_hash"] = (int(v) for v in blob[40:56].view("<u8"))
    return h


def parse(blob, **shape):
    """{name: numpy view into `blob`} of the blob's arrays (first axis: the env, for the per-env ones), the header's fields
    under "header".  `shape`: the keywords of _blob_layout that say which arrays the configuration has; n and the frames come
    from the header.  Every byte of the blob is accounted for."""
    blob = np.asarray(blob, np.uint8)
    h = header(blob)
    n = h["num_envs"]
    frames = h["obs_bytes_per_env"] if h["include_obs"] else None
    n_arrays, lengths = _walk(blob)
    want, names = _blob_layout(n, frames, **shape), _blob_names(frames, **shape)
    assert lengths == want and n_arrays == len(want) == len(names), (lengths, want)
    out, at = {"header": h}, HEADER_BYTES
    for (name, dtype), length in zip(names, lengths):
        v = blob[at + 8:at + 8 + length].view(dtype)
        if v.size != n and v.size % n == 0 and name not in ("errors", "reset_counts", "done_count", "perf"):
            v = v.reshape(n, -1)
        out[name] = v
        at += 8 + length
    assert at == blob.size
    return out


def _done_list(blob, shape):
    """(a writable copy of the blob, its done list, the number of entries that count -- None: the list is not valid)"""
    out = np.array(blob, np.uint8, copy=True)
    p = parse(out, **shape)
    if "done_list" not in p:
        return out, None, None
    n, count = p["header"]["num_envs"], int(p["done_count"][0])
    assert 0 <= count <= n, "done_count %d outside [0, %d]" % (count, n)
    return out, p["done_list"], (count if p["header"]["list_valid"] & 1 else None)


def canonical(blob, **shape):
    """The blob with the first done_count entries of the done list sorted and the rest of the list zeroed; a list the header
    does not call valid (list_valid bit 0) is zeroed whole.  Blobs of the games without a list come back unchanged."""
    out, lst, count = _done_list(blob, shape)
    if lst is not None:
        count = count or 0
        lst[:count] = np.sort(lst[:count])
        lst[count:] = 0
    return out


def permute_done_list(blob, perm, **shape):
    """A copy of the blob whose first done_count list entries are reordered: new[i] = old[perm[i]]"""
    out, lst, count = _done_list(blob, shape)
    assert lst is not None and count is not None, "the blob holds no valid done list"
    perm = np.asarray(list(perm), np.int64)
    assert np.array_equal(np.sort(perm), np.arange(count)), "perm must be a permutation of range(done_count)"
    lst[:count] = lst[:count][perm]
    return out
