"""The record sort in plain numpy: what pcv_sort_records must return, the rank-count rows, and the seeded generator of the
cases tests/sort_records_cases.py lists. No project code is imported here.

A record is a u32 key, optionally a payload of 2 words (12-byte records: key = rank << 8 | blue, red | green << 8 in the upper
half of the second payload word) or 4 words, and planes of words. The sort is stable by the TRUE rank: the key's rank field, or
map[predicted rank] & INDEX_MASK where a map is given; a map entry with REPLAY set makes the record's first payload word its
input index."""
import numpy as np

INDEX_MASK = 0x3FFFFFFF
REPLAY = 1 << 30
TILE = 8192         # records per tile of the 12-byte record sort
MAX_GROUPS = 1024   # sort workgroups at most
X_TAG = 0xA5000000  # first payload word = input index ^ X_TAG: a replayed record (word = index) is told from one left alone


def geometry(n):
    """(groups, chunk) of the 12-byte record sort: chunks of whole tiles, as few tiles per chunk as 1 024 workgroups allow."""
    tiles = -(-n // TILE)
    per_group = max(1, -(-tiles // MAX_GROUPS))
    chunk = per_group * TILE
    return max(1, -(-n // chunk)), chunk


def rank_shift(vec):
    return 8 if vec is not None and vec.shape[1] == 2 else 0


def predicted(keys, vec):
    return keys >> np.uint32(rank_shift(vec))


def rows_truth(keys, vec, map_entries):
    """rows[g][b]: keys of chunk g whose predicted rank is b."""
    groups, chunk = geometry(len(keys))
    pred = predicted(keys, vec).astype(np.int64)
    rows = np.zeros((groups, map_entries), dtype=np.uint32)
    for g in range(groups):
        rows[g] = np.bincount(pred[g * chunk:(g + 1) * chunk], minlength=map_entries)
    return rows


def sort_truth(keys, key_bits, vec=None, planes=(), map=None, color=None, color_stride=3):
    """-> dict(keys, vec, planes, order, true): the sorted arrays, the input index of every sorted slot and the true ranks (input
    order). `color` (n * color_stride bytes): the records come without colour and the sort joins it."""
    keys = np.asarray(keys, dtype=np.uint32)
    n = len(keys)
    shift = rank_shift(vec)
    pred = keys >> np.uint32(shift)
    if map is not None:
        entry = np.asarray(map, dtype=np.uint32)[pred]
        true = entry & np.uint32(INDEX_MASK)
        replay = (entry & np.uint32(REPLAY)) != 0
    else:
        true = pred & np.uint32((1 << key_bits) - 1)
        replay = np.zeros(n, dtype=bool)
    order = np.argsort(true, kind="stable")
    out_vec = None
    if vec is not None:
        out_vec = np.array(vec, dtype=np.uint32, copy=True)
        out_vec[replay, 0] = np.arange(n, dtype=np.uint32)[replay]
    low = keys & np.uint32((1 << shift) - 1)  # the colour byte of a 12-byte record
    if color is not None:
        c = np.asarray(color, dtype=np.uint8).reshape(n, color_stride).astype(np.uint32)
        low = low | c[:, 2]
        out_vec[:, 1] |= (c[:, 0] | (c[:, 1] << np.uint32(8))) << np.uint32(16)
    if map is not None:
        out_keys = (true << np.uint32(shift)) | low
    else:
        out_keys = keys | low  # bits outside the rank field travel
    return {"keys": out_keys[order], "vec": None if out_vec is None else out_vec[order],
            "planes": [np.asarray(p, dtype=np.uint32)[order] for p in planes], "order": order, "true": true}


def input_index_at(vec_row_or_plane_word, n, has_vec):
    """The input index a record names: from its first payload word (replayed: the index itself), else from plane 0."""
    w = int(vec_row_or_plane_word)
    if has_vec:
        return w ^ X_TAG if (w ^ X_TAG) < n else w
    return (w * PLANE_INV[0]) & 0xFFFFFFFF


def first_difference(want, got, what, truth, got_vec, got_plane0):
    """None, or a message naming the first sorted slot at which `got` differs: the input index expected there and the one found."""
    want, got = np.asarray(want), np.asarray(got)
    if want.shape == got.shape and np.array_equal(want, got):
        return None
    if want.shape != got.shape:
        return f"{what}: shape {got.shape}, expected {want.shape}"
    diff = want != got
    slot = int(np.argmax(diff.reshape(len(want), -1).any(axis=1)))
    n = len(want)
    found = None
    if got_vec is not None:
        found = input_index_at(got_vec[slot][0], n, True)
    elif got_plane0 is not None:
        found = input_index_at(got_plane0[slot], n, False)
    return (f"{what}: first difference at sorted slot {slot} of {n}: expected input index {int(truth['order'][slot])} "
            f"(true rank {int(truth['true'][truth['order'][slot]])}), found the record of input index {found}; "
            f"want {want[slot]}, got {got[slot]}")


# plane w of record i = i * PLANE_MUL[w] + PLANE_ADD[w] (mod 2^32): odd multipliers, so the words of a plane are distinct
PLANE_MUL = [2654435761, 40503 * 2 + 1, 2246822519, 3266489917, 668265263, 374761393, 0x9E3779B1, 0x85EBCA6B]
PLANE_ADD = [0, 0x01000193, 0x7F4A7C15, 12345, 0xDEADBEEF, 77, 0x10000001, 0xFFFFFFFE]
PLANE_INV = [pow(m, -1, 1 << 32) for m in PLANE_MUL]


def _true_ranks(rng, n, T, mode, distinct_limit):
    """Desired true ranks of the n records, input order. `distinct_limit`: how many different values a map can produce."""
    if mode == "random":  # some true ranks stay empty
        k = max(1, min(T - T // 4, distinct_limit))
        used = rng.permutation(T)[:k] if T <= (1 << 20) else np.unique(rng.integers(0, T, min(k, 2 * n + 2)))
        return used[rng.integers(0, len(used), n)]
    if mode == "one_low_digit":  # 60 % of the records share the lower 7 bits of their rank
        d0 = 0x35 % T
        t = rng.integers(0, T, n)
        heavy = rng.random(n) < 0.6
        t[heavy] = (t[heavy] & ~np.int64(0x7F)) | d0
        return t % T
    if mode == "few":  # 40 ranks in use
        used = rng.permutation(T)[:40]
        return used[rng.integers(0, len(used), n)]
    if mode == "same":
        return np.full(n, (T * 5) // 7, dtype=np.int64)
    if mode in ("sorted", "falling"):
        t = np.sort(rng.integers(0, T, n))
        return t if mode == "sorted" else t[::-1].copy()
    raise ValueError(mode)


def make_case(seed, n, key_bits, vec_words=2, nplanes=0, map_entries=0, replay=0.0, color_stride=0, ranks="random"):
    """-> dict(keys, vec, planes, map, color): the inputs of one sort. vec_words 0, 2 or 4. With a map (map_entries > 0) the keys
    carry predicted ranks < map_entries and the map is many-to-one onto [0, 2^key_bits), not monotone, with entries no record
    uses and true ranks nothing maps to; `replay`: share of the map entries that carry the replay mark. color_stride 3 or 4: the
    colour comes in an array of its own, the keys as rank << 8."""
    rng = np.random.default_rng(seed)
    T = min(1 << key_bits, 1 << 30) if map_entries else 1 << key_bits
    limit = max(1, map_entries // 2) if map_entries else T
    if ranks in ("sorted", "falling", "one_low_digit") and map_entries:
        limit = map_entries  # (these take any rank: the case gives the map room for all of them)
    true = np.asarray(_true_ranks(rng, n, T, ranks, limit), dtype=np.int64)
    map_arr = None
    if map_entries:
        used = np.unique(true)
        assert len(used) <= map_entries, "the map cannot produce that many true ranks"
        extra = map_entries - len(used)
        pool = np.concatenate([used, rng.integers(0, T, 3)])  # a few true ranks that only unused entries map to
        values = np.concatenate([used, pool[rng.integers(0, len(pool), extra)]])
        # entries the records use: one per true rank in use at least, and three quarters of the others
        in_use = np.concatenate([np.ones(len(used), dtype=bool), rng.random(extra) < 0.75])
        perm = rng.permutation(map_entries)
        values, in_use = values[perm], in_use[perm]
        usable = np.flatnonzero(in_use)
        by_value = usable[np.argsort(values[usable], kind="stable")]
        sorted_values = values[by_value]
        lo = np.searchsorted(sorted_values, true, side="left")
        hi = np.searchsorted(sorted_values, true, side="right")
        pred = by_value[lo + (rng.random(n) * (hi - lo)).astype(np.int64)]  # one of the entries that map to the record's rank
        map_arr = values.astype(np.uint32)
        if replay:
            map_arr[rng.random(map_entries) < replay] |= np.uint32(REPLAY)
        assert np.array_equal(map_arr[pred] & np.uint32(INDEX_MASK), true.astype(np.uint32))
    else:
        pred = true
    i = np.arange(n, dtype=np.uint32)
    compact = vec_words == 2
    keys = pred.astype(np.uint32)
    color = None
    if compact:
        keys = keys << np.uint32(8)
        if color_stride:
            color = rng.integers(0, 256, n * color_stride, dtype=np.uint8)
        else:
            keys |= rng.integers(0, 256, n, dtype=np.uint32)
    vec = None
    if vec_words:
        vec = np.empty((n, vec_words), dtype=np.uint32)
        vec[:, 0] = i ^ np.uint32(X_TAG)
        if compact:
            vec[:, 1] = (i * np.uint32(7) + np.uint32(3)) & np.uint32(0xFFFF)
            if not color_stride:
                vec[:, 1] |= rng.integers(0, 1 << 16, n, dtype=np.uint32) << np.uint32(16)
        else:
            vec[:, 1], vec[:, 2], vec[:, 3] = ~i, i * np.uint32(2654435761), i + np.uint32(0x1000)
    planes = [i * np.uint32(PLANE_MUL[w]) + np.uint32(PLANE_ADD[w]) for w in range(nplanes)]
    return {"keys": keys, "vec": vec, "planes": planes, "map": map_arr, "color": color}
