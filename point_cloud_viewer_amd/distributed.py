"""Multi-GPU octree build: shard by level-2 bucket, ONE all-to-all(v), independent subtree builds.

The reference is single-process (rayon tasks over nodes, src/octree/generation.rs:152-193). Subtrees are independent of
each other, which is what this module exploits across the GPUs of one node:

  1. every rank holds a contiguous slice of the input (rank order == input order);
  2. the bucket of a point — its level-1 and level-2 octant digits, 64 buckets — needs only the point and the GLOBAL
     root cube (ChildIndex::from_bounding_cube node.rs:34-42 plus one encode/decode step of the chain), so each rank
     computes it locally (HIP) together with the 64 bucket counts; one tiny all-reduce makes the counts global;
  3. from the global counts every rank derives the same plan: which level-1 nodes the global tree splits
     (count > capacity && child edge > resolution, generation.rs:128-150), and a bin-packing (largest first) of the
     buckets onto ranks — whole octants where the level-1 node stays a leaf. Gaussian-cluster clouds put very different
     numbers of points into the 8 root octants; 64 buckets even that out (SURVEY §8e "skew");
  4. a stable partition by owner followed by one grouped send/recv round (RCCL: a single ncclGroup == one
     all-to-all(v) over xGMI; planes x, y, z, rgb[, intensity]) routes every point to its owner. Receivers concatenate
     in source-rank order, so each bucket's stream stays in global input order — the property that makes per-node
     point order identical to the reference;
  5. each rank runs the ordinary build on what it received, with the GLOBAL bounding box and the global split
     decision for the level-1 nodes. Everything from level 2 down is exactly the single-GPU result;
  6. the every-8th promotion (generation.rs:195-253) into a level-1 node and into the root runs over streams that
     span ranks: the ranks all-reduce the lengths of their level-1/level-2 streams (72 numbers) between the topology
     and the encode phase, which fixes every promoted point's global slot. Each rank then writes its points into
     global-size top nodes (other slots zero), and one small all-reduce(sum) of those bytes (<= 9 nodes, a few MB)
     finishes the root and the level-1 nodes on every rank. No other collective touches point data.

The backend is pluggable so that the routing/merge logic can be exercised on CPU tensors with the gloo backend
(tests/test_distributed_cpu.py injects a host backend); the product backend is HIP (`HipBackend`).
"""
import numpy as np

from . import octree as _oct

DEFAULT_MAX_POINTS_PER_NODE = 100000  # generation.rs:37


def _ceil8(v):
    return (int(v) + 7) // 8


def plan_buckets(global_counts, world, max_points_per_node, level1_can_split, mode="buckets"):
    """(rank_of_bucket[64], split_mask) from the GLOBAL bucket counts — pure and deterministic, every rank computes the
    same plan. mode "buckets" (the skew remedy of SURVEY §8e): units are single buckets below level-1 nodes the global
    tree splits, whole octants otherwise; units go largest-first to the least-loaded rank (ties: lower bucket, lower
    rank). mode "octants" (BASELINE north_star: shard by the top-3-bit prefix): root octant c belongs to rank c % world,
    whatever it holds. The finished octree is the same either way; only the load balance differs."""
    g = np.asarray(global_counts, dtype=np.int64).reshape(8, 8)
    octant = g.sum(axis=1)
    units, split_mask = [], 0
    for c in range(8):
        if level1_can_split and octant[c] > max_points_per_node:
            split_mask |= 1 << c
            units += [(int(g[c, d]), [c * 8 + d]) for d in range(8) if g[c, d] > 0]
        elif octant[c] > 0:
            units.append((int(octant[c]), list(range(c * 8, c * 8 + 8))))
    if mode == "octants":
        return np.repeat(np.arange(8, dtype=np.uint8) % world, 8), split_mask
    if mode != "buckets":
        raise ValueError("shard mode must be 'buckets' or 'octants'")
    rank_of = np.zeros(64, dtype=np.uint8)
    loads = [0] * world
    for weight, buckets in sorted(units, key=lambda u: (-u[0], u[1][0])):
        r = min(range(world), key=lambda k: (loads[k], k))
        loads[r] += weight
        rank_of[buckets] = r
    return rank_of, split_mask


def top_layout(l1, l2, split_mask):
    """Global streams of the top of the tree from the summed local stream lengths: offsets of every level-2 node's
    promoted segment inside its level-1 node's stream, of every level-1 node's inside the root's (SURVEY Appendix A:
    |pre(inner)| = sum over children of ceil(|pre(child)| / 8))."""
    l1_stream, l1_offset, l2_offset = [0] * 8, [0] * 8, [0] * 64
    for c in range(8):
        if (split_mask >> c) & 1:
            acc = 0
            for d in range(8):
                l2_offset[c * 8 + d] = acc
                acc += _ceil8(l2[c * 8 + d])
            l1_stream[c] = acc
        else:
            l1_stream[c] = int(l1[c])
    acc = 0
    for c in range(8):
        l1_offset[c] = acc
        acc += _ceil8(l1_stream[c])
    return dict(root_points=acc, l1_stream=l1_stream, l1_offset=l1_offset, l2_offset=l2_offset)


def top_nodes(layout, encodings, has_intensity):
    """Finished root + level-1 nodes described by a layout: [(name, level, digit, num_points, encoding, xyz_off, rgb_off,
    int_off)] and the total byte size of the buffer that holds their xyz | rgb | intensity bytes. A cloud without points has no
    node at all, the root included (like the one-GPU build of an empty cloud): gather() is empty and write_dir writes meta.pb
    alone."""
    bpc = {1: 1, 2: 2, 3: 4, 4: 8}
    specs = [("r", 0, 0, layout["root_points"])] if layout["root_points"] > 0 else []
    for c in range(8):
        s = layout["l1_stream"][c]
        if s > 0:
            specs.append((f"r{c}", 1, c, s - _ceil8(s)))
    out, off = [], 0
    for name, level, digit, npts in specs:
        enc = int(encodings[level])
        xyz = npts * 3 * bpc[enc]
        out.append(dict(name=name, level=level, digit=digit, num_points=npts, encoding=enc, xyz=(off, xyz),
                        rgb=(off + xyz, npts * 3), intensity=(off + xyz + npts * 3, npts * 4 if has_intensity else 0)))
        off += xyz + npts * 3 + (npts * 4 if has_intensity else 0)
        off = (off + 15) & ~15
    return out, off


class HipBackend:
    """Device work for the sharded build, all through the C ABI (no CPU fallback)."""

    def __init__(self, ctx, device):
        import torch
        self.torch = torch
        self.ctx = ctx
        self.device = device

    def aabb(self, x, y, z):
        return self.ctx.aabb_reduce(x, y, z)

    def level_table(self, resolution, bbox):
        """(max_level, edges, encodings) of the global cube (PositionEncoding::new codec.rs:31-40)."""
        return _oct.level_table(bbox.min, bbox.max, resolution)

    def buckets(self, resolution, bbox, x, y, z, rgb=None, with_state=False):
        """(bucket per point, 64 counts[, level-1 chain state]): one HIP kernel (two chain levels + wave-aggregated
        histogram; the state is four 4-byte planes: the Float32 level-1 codes and octant digit | rgb)."""
        return self.ctx.route_buckets(resolution, bbox, x, y, z, rgb, with_state)

    def route_plan(self, resolution, bbox, x, y, z, octants_only=False):
        """Two-pass routing, first pass: (bucket bytes, per-tile bucket histograms, 64 counts) — no state is written.
        octants_only (shard mode "octants"): the level-1 digit alone, three comparisons per point. The two work arrays are
        kept across builds (a steady stream of equally sized slices allocates nothing)."""
        out = self.ctx.route_plan(resolution, bbox, x, y, z, octants_only, getattr(self, "_plan_buffers", None))
        self._plan_buffers = out[:2]
        return out

    def route_scatter(self, resolution, bbox, x, y, z, rgb, intensity, bucket, tile_hist, rank_of_bucket, dsts):
        """Second pass: the level-1 state computed again and stored straight into the owners' buffers."""
        self.ctx.route_scatter(resolution, bbox, x, y, z, rgb, bucket, tile_hist, rank_of_bucket, dsts, intensity)

    def partition(self, bucket, rank_of_bucket, planes, dsts):
        """Stable partition of the planes by owner straight into the destination views (count / scan / scatter)."""
        self.ctx.partition_by_owner(bucket, planes, dsts, rank_of_bucket)

    def after_torch(self):
        """Order the library's stream after torch's current stream: the exchange (RCCL) and torch fills run there, and
        `work.wait()` of an RCCL op only blocks that stream, not the host (the context owns a different stream)."""
        self.ctx.wait_torch()

    def before_torch(self):
        """Order torch's current stream after the library's queued work (asynchronous node copies)."""
        self.ctx.signal_torch()

    def build_begin(self, resolution, bbox, x, y, z, rgb, intensity, max_points_per_node, force_split_level1):
        return self.ctx.build_begin(resolution, bbox, x, y, z, rgb, intensity, max_points_per_node, force_split_level1)

    def build_begin_routed(self, resolution, bbox, state, intensity, max_points_per_node, force_split_level1):
        return self.ctx.build_begin_routed(resolution, bbox, state, intensity, max_points_per_node, force_split_level1)


class ShardedOctree:
    """Result of a sharded build: this rank's subtrees (level >= 2) plus the finished root and level-1 nodes, which
    every rank holds after the top all-reduce."""

    def __init__(self, builder, local_tree, top, top_bytes, stage_ms, counts, plan, resolution, bbox):
        self.builder = builder
        self.resolution, self.bbox = resolution, bbox
        self.local = local_tree
        self.top = top              # list of node dicts (top_nodes)
        self.top_bytes = top_bytes  # uint8 tensor: xyz | rgb | intensity of the top nodes
        self._stage_ms = stage_ms
        self.counts = counts        # world x world matrix: counts[src][dst]
        self.plan = plan            # (rank_of_bucket, split_mask)
        self.bytes_per_row = 0      # exchange payload per point (set by the builder)

    @property
    def num_nodes_local(self):
        return self.local.num_nodes

    @property
    def stage_ms(self):
        ms = dict(self.local.stage_ms()) if hasattr(self.local, "stage_ms") else {}
        ms.update(self._stage_ms)
        return ms

    def free(self):
        if hasattr(self.local, "free"):
            self.local.free()

    def exchange_info(self):
        """What this rank moved through the all-to-all(v): rows and bytes sent to / received from OTHER ranks, the
        load balance of the plan (points owned per rank), and the stage times."""
        m = np.asarray(self.counts, dtype=np.int64)
        rank = self.builder.rank
        bpr = self.bytes_per_row
        sent = int(m[rank].sum() - m[rank, rank])
        recv = int(m[:, rank].sum() - m[rank, rank])
        owned = m.sum(axis=0)
        return {"ranks": int(m.shape[0]), "shard_mode": self.builder.shard_mode, "bytes_per_row": bpr,
                "rows_sent": sent, "rows_received": recv, "bytes_sent": sent * bpr, "bytes_received": recv * bpr,
                "points_owned_per_rank": [int(v) for v in owned],
                "imbalance_max_over_mean": round(float(owned.max() / max(owned.mean(), 1.0)), 4),
                "ms": {k: round(float(v), 3) for k, v in self._stage_ms.items()}}

    def top_dict(self):
        """The finished root and level-1 nodes as {name: node dict} (host bytes)."""
        raw = self.top_bytes.cpu().numpy() if hasattr(self.top_bytes, "cpu") else np.asarray(self.top_bytes)
        out = {}
        for nd in self.top:
            cut = lambda k: raw[nd[k][0]:nd[k][0] + nd[k][1]].tobytes()
            out[nd["name"]] = dict(id=(nd["level"] << 56, nd["digit"]), num_points=nd["num_points"],
                                   encoding=nd["encoding"], level=nd["level"], xyz=cut("xyz"), rgb=cut("rgb"),
                                   intensity=cut("intensity"))
        return out

    def write_dir(self, directory, dst=0):
        """The reference's output directory from all ranks (shared file system): every rank writes the node files of
        its own subtrees, `dst` adds the finished root / level-1 nodes and meta.pb for the gathered node table."""
        import os
        dist = self.builder.dist
        os.makedirs(directory, exist_ok=True)
        self.local.write_nodes(directory, 2)
        mine = []
        for i in range(self.local.num_nodes):
            nd = self.local.node(i)
            if nd.level >= 2:
                mine.append((nd.id_high, nd.id_low, nd.num_points, nd.encoding))
        gathered = [None] * dist.get_world_size() if dist.get_rank() == dst else None
        dist.gather_object(mine, gathered, dst=dst)
        if dist.get_rank() == dst:
            nodes = []
            for name, nd in self.top_dict().items():
                nodes.append((nd["id"][0], nd["id"][1], nd["num_points"], nd["encoding"]))
                if nd["num_points"]:  # node_writer.rs:78-89: empty nodes have no files
                    for ext in ("xyz", "rgb", "intensity"):
                        if nd[ext]:
                            with open(os.path.join(directory, f"{name}.{ext}"), "wb") as f:
                                f.write(nd[ext])
            for part in gathered:
                nodes += part
            nodes.sort(key=lambda t: (t[0], t[1]))  # (level, index): the reference's order is nondeterministic
            _oct.write_meta(directory, self.resolution, self.bbox.min, self.bbox.max, nodes)
        dist.barrier()

    def gather(self, dst=0):
        """Merge all ranks' node dictionaries on `dst` (tests, directory writing): the top nodes come from the
        all-reduced buffer, every deeper node is built by exactly one rank."""
        dist = self.builder.dist
        local = {k: v for k, v in self.local.to_dict().items() if v["level"] >= 2}
        gathered = [None] * dist.get_world_size() if dist.get_rank() == dst else None
        dist.gather_object(local, gathered, dst=dst)
        if dist.get_rank() != dst:
            return None
        merged = self.top_dict()
        for part in gathered:
            for name, nd in part.items():
                assert name not in merged, f"node {name} built by two ranks"
                merged[name] = dict(nd)
        return merged


class ShardedOctreeBuilder:
    def __init__(self, ctx, dist, device, backend=None, compress_exchange=True, shard_mode="buckets"):
        import torch
        self.torch = torch
        self.dist = dist
        self.shard_mode = shard_mode  # "buckets" (64 level-2 buckets bin-packed) or "octants" (octant c -> rank c % N)
        # ship the level-1 chain state (Float32 codes + octant digit | rgb: four 4-byte planes, 16 B) instead of raw f64
        # coordinates + rgb (27 B) whenever level 1 of the global cube is Float32-encoded; bit-identical either way
        self.compress_exchange = compress_exchange
        self.device = device
        self.rank = dist.get_rank()
        self.world = dist.get_world_size()
        if self.world > 8:
            raise ValueError("the sharded build addresses at most 8 ranks (one node)")
        self.backend = backend or HipBackend(ctx, device)
        # send / receive planes of the exchange, kept across builds; a build's result views the receive planes only until the
        # routed build has read them (pcv_build_begin_routed copies nothing, but finish() is synchronous), so the next build
        # may overwrite them
        self._exchange_buffers = {}

    # -- global bounding box (== find_bounding_box over the whole input, generation.rs:256-270) --
    def global_bbox(self, x, y, z):
        torch, dist = self.torch, self.dist
        self._after_torch()
        bmin, bmax = self.backend.aabb(x, y, z)
        n_local = x.numel() if hasattr(x, "numel") else len(x)
        big = np.finfo(np.float64).max
        if n_local == 0:  # an empty slice must not pull the box towards Aabb::zero()
            bmin, bmax = np.full(3, big), np.full(3, -big)
        # ONE collective and one read-back: min over [lo, -hi] (negation is exact), 6 numbers
        v = torch.tensor(np.concatenate([np.asarray(bmin, dtype=np.float64), -np.asarray(bmax, dtype=np.float64)]),
                         dtype=torch.float64, device=self.device)
        dist.all_reduce(v, op=dist.ReduceOp.MIN)
        h = v.cpu().numpy()
        return _oct.Aabb(h[:3].copy(), -h[3:])

    def _after_torch(self):
        if hasattr(self.backend, "after_torch"):
            self.backend.after_torch()

    def _before_torch(self):
        if hasattr(self.backend, "before_torch"):
            self.backend.before_torch()

    def _sum_i64(self, values):
        """All-reduce(sum) of a small host vector of int64."""
        t = self.torch.tensor(np.asarray(values, dtype=np.int64), device=self.device)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.SUM)
        return t.cpu().numpy()

    def _route(self, bucket, rank_of_bucket, matrix, planes, scatter=None):
        """Partition by owner and exchange: rows for rank r go to a send buffer, own rows directly into the receive
        buffer; ONE grouped send/recv round moves everything else (RCCL: one ncclGroup == one all-to-all(v)).
        matrix[src][dst] = rows src sends to dst; planes: dict name -> row-aligned tensor; returns the received planes
        under the same names."""
        torch, dist = self.torch, self.dist
        world, rank = self.world, self.rank
        send_counts = [int(v) for v in matrix[rank]]
        recv_counts = matrix[:, rank]
        n_recv = int(recv_counts.sum())
        n_local = int(sum(send_counts))
        send_off = np.concatenate([[0], np.cumsum(send_counts)]).astype(np.int64)
        recv_off = np.concatenate([[0], np.cumsum(recv_counts)]).astype(np.int64)
        names = list(planes)

        def rows_of(side, k, p, rows):
            # exchange buffers kept across builds (VERDICT r05 #2c): a view of the builder's block when it is big enough
            key = (side, k, p.dtype, tuple(p.shape[1:]))
            have = self._exchange_buffers.get(key)
            if have is None or int(have.shape[0]) < rows or have.device != p.device:
                have = torch.empty((max(rows, 1),) + tuple(p.shape[1:]), dtype=p.dtype, device=p.device)
                self._exchange_buffers[key] = have
            return have[:rows]

        send = {k: rows_of("send", k, planes[k], n_local) for k in names}
        recv = {k: rows_of("recv", k, planes[k], n_recv) for k in names}
        dsts = []
        for r in range(world):
            buf, off, cnt = (recv, recv_off[rank], send_counts[rank]) if r == rank else (send, send_off[r], send_counts[r])
            dsts.append([buf[k][off:off + cnt] for k in names])
        if scatter is not None:  # two-pass routing: the planes do not exist yet, `scatter` computes them into the buffers
            scatter(rank_of_bucket, [dict(zip(names, row)) for row in dsts])
        else:
            self.backend.partition(bucket, rank_of_bucket, [planes[k] for k in names], dsts)
        ops = []
        for k in names:
            for peer in range(world):
                if peer == rank:
                    continue
                if send_counts[peer] > 0:
                    ops.append(dist.P2POp(dist.isend, send[k][send_off[peer]:send_off[peer + 1]], peer))
                if recv_counts[peer] > 0:
                    ops.append(dist.P2POp(dist.irecv, recv[k][recv_off[peer]:recv_off[peer + 1]], peer))
        if ops:
            for w in dist.batch_isend_irecv(ops):
                w.wait()
        # RCCL's wait() orders torch's current stream only; the build reads `recv` on the library's own stream
        self._after_torch()
        return recv

    def build(self, resolution, bbox, x, y, z, rgb, intensity=None, max_points_per_node=0):
        torch = self.torch
        world = self.world
        cap = max_points_per_node or DEFAULT_MAX_POINTS_PER_NODE
        timed = self.device.type == "cuda" if hasattr(self.device, "type") else False
        marks = []

        def mark():
            if timed:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                marks.append(e)

        mark()
        self._after_torch()  # the caller's tensors were produced on torch's stream
        max_level, edges, encodings = self.backend.level_table(resolution, bbox)
        can_split = max_level >= 2 and edges[1] > resolution
        # 1. buckets + global plan
        compressed = bool(self.compress_exchange and max_level >= 1 and int(encodings[1]) == 3)  # Float32 level 1
        two_pass = compressed and hasattr(self.backend, "route_plan") and int(x.shape[0]) > 0
        scatter = None
        if two_pass:
            # the state never exists in input order: pass 1 leaves bucket bytes + tile histograms, pass 2 (inside _route, once
            # the plan is known) writes every point's state straight into its owner's buffer; `planes` only describes the rows
            if self.shard_mode == "octants":  # the owner is a function of the level-1 digit: no level step in the plan
                bucket, tile_hist, counts = self.backend.route_plan(resolution, bbox, x, y, z, True)
            else:
                bucket, tile_hist, counts = self.backend.route_plan(resolution, bbox, x, y, z)
            planes = {k: torch.empty(0, dtype=torch.int32, device=self.device) for k in ("cx", "cy", "cz", "oct_rgb")}
            if intensity is not None:
                planes["intensity"] = torch.empty(0, dtype=intensity.dtype, device=self.device)

            def scatter(rank_of, dsts):
                self.backend.route_scatter(resolution, bbox, x, y, z, rgb, intensity, bucket, tile_hist, rank_of, dsts)
        elif compressed:
            bucket, counts, state = self.backend.buckets(resolution, bbox, x, y, z, rgb, True)
            planes = dict(state)
        else:
            bucket, counts = self.backend.buckets(resolution, bbox, x, y, z)
            planes = {"x": x, "y": y, "z": z, "color": rgb}
        if intensity is not None and not two_pass:
            planes["intensity"] = intensity
        row_bytes = sum(int(p.element_size()) * (int(p.numel()) // max(int(p.shape[0]), 1) if int(p.shape[0]) else
                                                  int(np.prod(p.shape[1:], dtype=np.int64))) for p in planes.values())
        # one all-gather of the 64 local counts gives every rank the global counts AND the whole send matrix
        if world == 1:  # (a one-rank group: the gathered table is the local one; RCCL would only add a launch and a sync)
            per_rank = np.asarray(counts, dtype=np.int64).reshape(1, 64)
        else:
            mine = torch.tensor(np.asarray(counts, dtype=np.int64), device=self.device)
            every = torch.empty((world, 64), dtype=torch.int64, device=self.device)
            self.dist.all_gather(list(every.unbind(0)), mine)  # rows of ONE tensor: one read-back instead of a stack + copy
            per_rank = every.cpu().numpy()  # per_rank[src][bucket]
        rank_of_bucket, split_mask = plan_buckets(per_rank.sum(axis=0), world, cap, can_split, self.shard_mode)
        matrix = np.stack([np.bincount(rank_of_bucket, weights=per_rank[src], minlength=world) for src in range(world)])
        matrix = matrix.astype(np.int64)  # matrix[src][dst]
        # 2. the exchange
        recv = self._route(bucket, rank_of_bucket, matrix, planes, scatter)
        del bucket, planes, scatter
        mark()
        # 3. local topology, then the global streams of the top of the tree
        if compressed:
            pending = self.backend.build_begin_routed(resolution, bbox, {k: recv[k] for k in ("cx", "cy", "cz", "oct_rgb")},
                                                      recv.get("intensity"), cap, split_mask)
        else:
            pending = self.backend.build_begin(resolution, bbox, recv["x"], recv["y"], recv["z"], recv["color"],
                                               recv.get("intensity"), cap, split_mask)
        l1, l2, _ = pending.top_streams()
        for c in range(8):
            if (split_mask >> c) & 1:
                l1[c] = 0  # a split level-1 node's stream is the sum over its level-2 nodes, derived below
        summed = self._sum_i64(np.concatenate([l1, l2]))
        layout = top_layout(summed[:8], summed[8:], split_mask)
        tree = pending.finish(layout)
        mark()
        # 4. finish the root and the level-1 nodes: sum of every rank's sparsely filled global-size nodes
        specs, nbytes = top_nodes(layout, encodings, intensity is not None)
        top = torch.zeros(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        self._after_torch()  # the zero fill runs on torch's stream, the node copies on the library's
        index_of = {}
        for i in range(min(tree.num_nodes, 9)):
            nd = tree.node(i)
            if nd.level <= 1:
                index_of[_oct.node_name(nd.id_high, nd.id_low)] = i
        copies = []
        bytes_per_code = {1: 1, 2: 2, 3: 4, 4: 8}
        for nd in specs:
            i = index_of.get(nd["name"])
            if i is not None:
                # a local top node must fill exactly its slot of the global layout: the batched copy below only knows offsets,
                # a node longer than its slot would overwrite its neighbours in the all-reduce buffer
                info = tree.node(i)
                have = {"xyz": info.num_points * 3 * bytes_per_code[int(info.encoding)], "rgb": info.num_points * 3,
                        "intensity": info.num_points * 4 if intensity is not None else 0}
                for key in ("xyz", "rgb", "intensity"):
                    if nd[key][1] and have[key] != nd[key][1]:
                        raise RuntimeError(f"sharded build: local top node {nd['name']} has {have[key]} {key} bytes, "
                                           f"its slot in the global layout {nd[key][1]}")
                copies.append((i, [nd[key] if nd[key][1] else None for key in ("xyz", "rgb", "intensity")]))
        if copies and hasattr(tree, "copy_nodes_into"):
            # one ABI call for all top nodes and file kinds
            tree.copy_nodes_into([(i, tuple(None if r is None else r[0] for r in ranges)) for i, ranges in copies], top)
        else:  # host test backends
            for i, ranges in copies:
                for which, r in enumerate(ranges):
                    if r is not None:
                        tree.copy_node_into(i, which, top[r[0]:r[0] + r[1]])
        self._before_torch()  # the node copies are queued on the library's stream, the collective runs on torch's
        if world > 1:
            self.dist.all_reduce(top, op=self.dist.ReduceOp.SUM)
        mark()
        ms = {}
        if timed:
            marks[-1].synchronize()
            ms = {"exchange": marks[0].elapsed_time(marks[1]), "local_build": marks[1].elapsed_time(marks[2]),
                  "top_merge": marks[2].elapsed_time(marks[3])}
        out = ShardedOctree(self, tree, specs, top, ms, matrix, (rank_of_bucket, split_mask), resolution, bbox)
        out.bytes_per_row = row_bytes
        return out
