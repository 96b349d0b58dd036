"""Host-side mirror of the reference's octree-build surface over the C ABI (thin; all work is in HIP).

Reference names kept: `build_octree(output_directory, resolution, bounding_box, input, attributes)`
(src/octree/generation.rs:289-295), `NodeId` Display/parse (src/octree/node.rs:59-86), `Aabb`.
Inputs may be numpy arrays (host) or torch CUDA tensors (device-resident; zero copy).
"""
import ctypes as C
import os
import sys
import weakref

import numpy as np

from . import _lib as L


def _is_torch(a):
    return type(a).__module__.startswith("torch")


def node_name(id_high, id_low):
    """NodeId Display (node.rs:73-86): 'r' + octal index padded to `level` digits."""
    level = id_high >> 56
    index = ((id_high & ((1 << 56) - 1)) << 64) | id_low
    return "r" + "".join(str((index >> (3 * j)) & 7) for j in range(level - 1, -1, -1))


class Aabb:
    """geometry::Aabb (src/geometry/aabb.rs:13-27): mins/maxs are the inf/sup of the two corners."""

    def __init__(self, a, b):
        a = np.asarray(a, dtype=np.float64)
        b = np.asarray(b, dtype=np.float64)
        self.min = np.minimum(a, b)
        self.max = np.maximum(a, b)


class DeviceColumn:
    """A column on the device that another object owns (a LasCloud): pointer, elements and dtype. It goes wherever a torch
    device tensor goes (build, s2_split, Terrain.add_points, ...) for as long as its owner lives; numpy() downloads it."""

    def __init__(self, owner, name, ptr, size, dtype):
        self.owner, self.name, self.ptr, self.size, self.dtype = owner, name, ptr, int(size), np.dtype(dtype)

    @property
    def shape(self):
        return (self.size // 3, 3) if self.name == "color" else (self.size,)

    def numpy(self):
        return self.owner.read(self.name)


class _Buf:
    """Pointer + keep-alive for one input array."""

    def __init__(self, arr, dtype, what):
        self.keep = arr
        if arr is None:
            self.ptr, self.device, self.size = None, None, 0
            return
        if isinstance(arr, DeviceColumn):
            if arr.dtype != np.dtype(dtype):
                raise TypeError(f"{what}: expected {np.dtype(dtype)}, got {arr.dtype}")
            arr.owner._alive()
            self.ptr, self.device, self.size = arr.ptr, True, arr.size
            return
        if _is_torch(arr):
            import torch
            want = {np.float64: torch.float64, np.uint8: torch.uint8, np.float32: torch.float32,
                    np.uint64: torch.int64, np.uint32: torch.int32}[dtype]
            if arr.dtype != want and not (dtype is np.uint64 and arr.dtype == torch.uint64) and not (
                    dtype is np.uint32 and arr.dtype == torch.uint32):
                raise TypeError(f"{what}: expected torch dtype {want}, got {arr.dtype}")
            if not arr.is_contiguous():
                raise ValueError(f"{what}: tensor must be contiguous")
            self.ptr = arr.data_ptr()
            self.device = arr.is_cuda
            self.size = arr.numel()
        else:
            a = np.ascontiguousarray(arr, dtype=dtype)
            self.keep = a
            self.ptr = a.ctypes.data
            self.device = False
            self.size = a.size


def _attr_type_of(arr):
    """The type string of an attribute column, inferred from the array: (n,) of the ten scalar dtypes, (n, 3) u8 (u8vec3),
    (n, 3) f64 (f64vec3)."""
    shape = tuple(arr.shape)
    if _is_torch(arr):
        import torch
        names = {torch.uint8: "u8", torch.int8: "i8", torch.int16: "i16", torch.int32: "i32", torch.int64: "i64",
                 torch.float32: "f32", torch.float64: "f64"}
        for t, k in (("uint16", "u16"), ("uint32", "u32"), ("uint64", "u64")):
            if hasattr(torch, t):
                names[getattr(torch, t)] = k
        base = names.get(arr.dtype)
    else:
        dt = np.asarray(arr).dtype
        base = {("u", 1): "u8", ("u", 2): "u16", ("u", 4): "u32", ("u", 8): "u64", ("i", 1): "i8", ("i", 2): "i16", ("i", 4): "i32",
                ("i", 8): "i64", ("f", 4): "f32", ("f", 8): "f64"}.get((dt.kind, dt.itemsize))
    if base is None:
        raise TypeError(f"attribute: no attribute data type for dtype {arr.dtype}")
    if len(shape) == 1:
        return base
    if len(shape) == 2 and shape[1] == 3 and base in ("u8", "f64"):
        return base + "vec3"
    raise TypeError(f"attribute: shape {shape} of {base} is no attribute column; (n,) scalars, (n, 3) u8 or (n, 3) f64 are")


def _attributes(attrs, n, device):
    """dict name -> array | (array, type string) as the pcv_attribute list of a batch of n points that lives on the device or
    not -> (ctypes array or None, count, keep-alive)."""
    if not attrs:
        return None, 0, []
    out, keep = (L.Attribute * len(attrs))(), []
    for k, (name, col) in enumerate(attrs.items()):
        typ = None
        if isinstance(col, tuple):
            col, typ = col
        if isinstance(col, DeviceColumn):
            col.owner._alive()
            if not device and n > 0:
                raise ValueError("all point arrays must live in the same memory space")
            name_b = os.fsencode(name) if isinstance(name, str) else bytes(name)
            keep.extend((col, name_b))
            out[k].name, out[k].data_type, out[k].reserved, out[k].data = name_b, L.ATTR_TYPES[_attr_type_of(np.zeros(0, col.dtype))][0], 0, col.ptr
            continue
        if not _is_torch(col):
            col = np.asarray(col)
        typ = _attr_type_of(col) if typ is None else str(typ).lower()
        if typ not in L.ATTR_TYPES:
            raise L.PcvError(L.PCV_E_INVALID, f"Attribute data type invalid (attribute '{name}', type {typ!r})")
        code, dtype, comps = L.ATTR_TYPES[typ]
        if _is_torch(col):
            if not col.is_contiguous():
                raise ValueError(f"attribute '{name}': tensor must be contiguous")
            if bool(col.is_cuda) != bool(device) and n > 0:
                raise ValueError("all point arrays must live in the same memory space")
            nbytes, ptr = col.numel() * col.element_size(), col.data_ptr()
        else:
            if col.dtype.itemsize != np.dtype(dtype).itemsize:
                raise TypeError(f"attribute '{name}': dtype {col.dtype} is not of type {typ}")
            if device and n > 0:
                raise ValueError("all point arrays must live in the same memory space")
            col = np.ascontiguousarray(col)
            nbytes, ptr = col.nbytes, col.ctypes.data
        if nbytes != n * comps * np.dtype(dtype).itemsize:
            raise ValueError(f"attribute '{name}': {nbytes} bytes, {n} points of type {typ} need {n * comps * np.dtype(dtype).itemsize}")
        name_b = os.fsencode(name) if isinstance(name, str) else bytes(name)
        keep.extend((col, name_b))
        out[k].name, out[k].data_type, out[k].reserved, out[k].data = name_b, code, 0, ptr
    return out, len(attrs), keep


class Context:
    """One pcv_ctx: bound to one HIP device and stream, not thread-safe (include/pcv_hip.h).

    stream=None (or handle 0, which the C ABI cannot tell from NULL) gives the context its OWN non-blocking stream.
    Torch's default stream is handle 0 and therefore can never be shared: work queued by torch (or RCCL) that produces
    the context's inputs must be ordered with `wait_torch()` / `wait_stream(handle)` before the first call that reads
    it, and `signal_torch()` orders torch work after asynchronous context calls. Calls that return results to the host
    end with a stream synchronisation of their own."""

    def __init__(self, device=0, stream=None):
        self.lib = L.load_library()
        h = C.c_void_p()
        self.device = int(device)
        self.shares_stream = bool(stream)
        rc = self.lib.pcv_ctx_create(int(device), C.c_void_p(stream) if stream else None, C.byref(h))
        if rc != L.PCV_OK:
            raise L.PcvError(rc, f"pcv_ctx_create(device={device}) failed — is a HIP device visible?")
        self.handle = h
        self._children = weakref.WeakSet()  # octrees / shape sets that borrow this context's pool
        # every build of this context records its per-stage GPU times (PCV_BUILD_STAGE_TIMES: ~0.1 ms of stream time per
        # build); off, stage_ms() of a tree reports the total only. build(stage_times=...) overrides it per call.
        self.stage_times = False

    def trim(self):
        """Give the cached scratch blocks of the context's pool back to the driver (pcv_ctx_trim)."""
        self._check(self.lib.pcv_ctx_trim(self.handle))

    def pool_stats(self, reset_peak=False):
        """(bytes the device pool has handed out now, the most since the last reset) (pcv_ctx_pool_stats); reset_peak=True sets
        the high-water mark to the current figure after reading it."""
        live, peak = C.c_uint64(), C.c_uint64()
        self._check(self.lib.pcv_ctx_pool_stats(self.handle, C.byref(live), C.byref(peak), 1 if reset_peak else 0))
        return live.value, peak.value

    def set_pool_guard(self, mode, fill=0):
        """Test hook (pcv_ctx_set_pool_guard): 0 off; 1 every block of the device pool is handed out holding the byte `fill`;
        2 fenced with canary bytes on both sides as well. Only while nothing built on the context is alive; resets the report."""
        self._check(self.lib.pcv_ctx_set_pool_guard(self.handle, int(mode), int(fill)))

    def pool_guard_check(self):
        """Scan the fences of every live block (pcv_ctx_pool_guard_check); blocks are scanned on release anyway."""
        self._check(self.lib.pcv_ctx_pool_guard_check(self.handle))

    def pool_guard_report(self):
        """{"checked", "damaged", and of the first damaged block "bytes", "serial", "offset"} (pcv_ctx_pool_guard_report)."""
        v = [C.c_uint64() for _ in range(4)]
        off = C.c_int64()
        self._check(self.lib.pcv_ctx_pool_guard_report(self.handle, *[C.byref(x) for x in v], C.byref(off)))
        return {"checked": v[0].value, "damaged": v[1].value, "bytes": v[2].value, "serial": v[3].value, "offset": off.value}

    def pool_guard_selftest(self, nbytes, offset):
        """The guard shown to work on one block of nbytes, and one byte planted at pointer + offset (pcv_ctx_pool_guard_selftest)."""
        self._check(self.lib.pcv_ctx_pool_guard_selftest(self.handle, int(nbytes), int(offset)))

    def close(self):
        # query batches first: freeing an S2 batch reads its cloud (pcv_s2_query_free), so the cloud must still be there
        for child in sorted(getattr(self, "_children", []), key=lambda c: 0 if isinstance(c, QueryBatch) else 1):
            child.free()
        if getattr(self, "handle", None):
            self.lib.pcv_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_xray_chunk_bytes(self, nbytes=0):
        """Bytes of node images per download chunk of XrayTiles.write / node_pngs (pcv_ctx_set_xray_chunk_bytes; 0: the
        default of 64 MiB). A chunk holds at least one tile."""
        self._check(self.lib.pcv_ctx_set_xray_chunk_bytes(self.handle, int(nbytes)))

    def set_profiling(self, enabled=True):
        """Bracket kernel launches with HIP events on the ctx stream (see kernel_stats): True / 1 = every launch,
        "major" / 2 = only the kernels that pass over the whole cloud, False / 0 = off."""
        level = 2 if enabled in ("major", 2) else (1 if enabled else 0)
        self._check(self.lib.pcv_ctx_set_profiling(self.handle, level))

    def reset_kernel_stats(self):
        self._check(self.lib.pcv_ctx_reset_kernel_stats(self.handle))

    def kernel_stats(self):
        """{kernel name: (launches, total_ms)} accumulated since the last reset."""
        out = {}
        count = self.lib.pcv_ctx_kernel_stats(self.handle, -1, None, None, None)
        for k in range(count):
            name, launches, ms = C.c_char_p(), C.c_uint64(), C.c_double()
            self.lib.pcv_ctx_kernel_stats(self.handle, k, C.byref(name), C.byref(launches), C.byref(ms))
            out[name.value.decode()] = (launches.value, ms.value)
        return out

    def synchronize(self):
        """Wait for the work queued on the context's stream."""
        self._check(self.lib.pcv_ctx_synchronize(self.handle))

    def wait_stream(self, stream_handle):
        """Order the context's stream after what is queued on `stream_handle` (0 = the default stream) right now."""
        self._check(self.lib.pcv_ctx_wait_stream(self.handle, C.c_void_p(stream_handle) if stream_handle else None))

    def signal_stream(self, stream_handle):
        """Order work queued on `stream_handle` from now on after the context's work queued so far."""
        self._check(self.lib.pcv_ctx_signal_stream(self.handle, C.c_void_p(stream_handle) if stream_handle else None))

    def wait_torch(self):
        """wait_stream on torch's current stream of this device: call after torch / torch.distributed produced
        tensors the next context call reads."""
        import torch
        self.wait_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def signal_torch(self):
        import torch
        self.signal_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def _check(self, rc):
        if rc != L.PCV_OK:
            raise L.PcvError(rc, self.lib.pcv_last_error(self.handle).decode())

    def terrain_begin(self, bbox_min, bbox_max, **params):
        """An empty Terrain over the world box (pcv_terrain_begin); params: terrain_params' arguments, or params=a
        TerrainParams."""
        pr = params["params"] if "params" in params else terrain_params(**params)
        lo = (C.c_double * 3)(*[float(v) for v in bbox_min])
        hi = (C.c_double * 3)(*[float(v) for v in bbox_max])
        h = C.c_void_p()
        self._check(self.lib.pcv_terrain_begin(self.handle, C.byref(pr), lo, hi, C.byref(h)))
        return Terrain(self, h, pr)

    def map_tiles_begin(self, zoom, **params):
        """An empty MapTiles layer at `zoom` (pcv_maptiles_begin); params: map_tiles_params' arguments."""
        pr = map_tiles_params(zoom, **params)
        h = C.c_void_p()
        self._check(self.lib.pcv_maptiles_begin(self.handle, C.byref(pr), C.byref(h)))
        return MapTiles(self, h, pr)

    def terrain_open(self, directory):
        """The finished Terrain of a terrain directory (pcv_terrain_open_dir): what Terrain.write leaves, or any directory
        sdl_viewer --terrain reads. It serves tiles, heights, colors, info, write and OctreeResult.render(terrain=...)."""
        import json
        h = C.c_void_p()
        self._check(self.lib.pcv_terrain_open_dir(self.handle, os.fsencode(str(directory)), C.byref(h)))
        with open(os.path.join(str(directory), "meta.json")) as f:
            meta = json.load(f)
        iso = meta["world_from_terrain"]
        pr = terrain_params(tile_size=meta["tile_size"], resolution_m=meta["resolution_m"], origin=meta["origin"],
                            world_from_terrain=list(iso["translation"]) + list(iso["rotation"]))
        return Terrain(self, h, pr)

    def terrain_from_tiles(self, tile_size, world_from_terrain, origin, resolution_m, tiles, heights, colors):
        """A finished Terrain from tiles made elsewhere (pcv_terrain_from_tiles); the arguments are read_terrain's keys:
        tiles int32 [n, 2], heights float32 [n, T, T, 2], colors uint8 [n, T, T, 4], numpy arrays or torch device tensors.
        The tiles are stored ascending by (x, y)."""
        pr = terrain_params(tile_size=tile_size, resolution_m=resolution_m, origin=origin, world_from_terrain=world_from_terrain)
        terrain_check_params(pr)
        pos = np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 2))
        n, T = pos.shape[0], int(tile_size)
        bh, bc = _Buf(heights, np.float32, "heights"), _Buf(colors, np.uint8, "colors")
        if bh.size != n * T * T * 2 or bc.size != n * T * T * 4:
            raise L.PcvError(L.PCV_E_INVALID, f"{n} tiles of {T} x {T} vertices take {n * T * T * 2} heights and {n * T * T * 4} colour bytes, "
                                              f"got {bh.size} and {bc.size}")
        if bh.device != bc.device:
            raise ValueError("heights and colors must live in the same memory space")
        if bh.device:
            self.wait_torch()
        h = C.c_void_p()
        self._check(self.lib.pcv_terrain_from_tiles(self.handle, C.byref(pr), n, pos.ctypes.data, bh.ptr, bc.ptr,
                                                    L.MEM_DEVICE if bh.device else L.MEM_HOST, C.byref(h)))
        return Terrain(self, h, pr)

    def _points(self, x, y, z, color=None, intensity=None):
        bx, by, bz = _Buf(x, np.float64, "x"), _Buf(y, np.float64, "y"), _Buf(z, np.float64, "z")
        bc = _Buf(color, np.uint8, "color")
        bi = _Buf(intensity, np.float32, "intensity")
        n = bx.size
        if by.size != n or bz.size != n:
            raise ValueError("x, y, z must have the same length")
        devs = {b.device for b in (bx, by, bz, bc, bi) if b.ptr is not None}
        if len(devs) > 1:
            raise ValueError("all point arrays must live in the same memory space")
        stride = 3
        if color is not None:
            if bc.size == 4 * n and n > 0:
                stride = 4
            elif bc.size != 3 * n:
                raise ValueError("color must hold 3 or 4 bytes per point")
        if intensity is not None and bi.size != n:
            raise ValueError("intensity must hold one f32 per point")
        p = L.Points()
        p.n = n
        p.x, p.y, p.z = bx.ptr, by.ptr, bz.ptr
        p.color = bc.ptr
        p.color_stride = stride
        p.intensity = bi.ptr
        p.mem = L.MEM_DEVICE if (devs and devs.pop()) else L.MEM_HOST
        return p, (bx, by, bz, bc, bi)

    @staticmethod
    def _params(resolution, bmin, bmax, max_points_per_node=0, flags=0):
        pr = L.BuildParams()
        pr.resolution = float(resolution)
        if bmin is not None:
            for a in range(3):
                pr.bbox_min[a] = float(bmin[a])
                pr.bbox_max[a] = float(bmax[a])
        pr.max_points_per_node = int(max_points_per_node)
        pr.flags = int(flags)
        return pr

    # ---- the build -------------------------------------------------------------------------------
    def build(self, resolution, bounding_box, x, y, z, color, intensity=None, max_points_per_node=0,
              speculate_depth=True, single_chain=None, check_resolve=False, stage_times=None):
        """build_octree up to (not including) the file writes. bounding_box=None computes it on the
        device (== build_octree_from_file's find_bounding_box pass). single_chain: None = the library decides (from
        2^22 points on), True = force the single-chain build, False = exact two-chain pipeline; speculate_depth=False
        additionally computes and sorts full-depth keys. The result is identical in every mode. check_resolve: the
        single-chain build compares the device's rank map with the host's entry by entry (PCV_BUILD_CHECK_RESOLVE).
        stage_times: record the GPU time of every stage for stage_ms() (PCV_BUILD_STAGE_TIMES: ~0.1 ms of stream time per
        build; without it stage_ms() reports the total only); None = the context's `stage_times` attribute."""
        p, keep = self._points(x, y, z, color, intensity)
        flags = 0 if speculate_depth else L.BUILD_NO_SPECULATION
        if check_resolve:
            flags |= L.BUILD_CHECK_RESOLVE
        if self.stage_times if stage_times is None else stage_times:
            flags |= L.BUILD_STAGE_TIMES
        if single_chain is True:
            flags |= L.BUILD_FORCE_SINGLE_CHAIN
        elif single_chain is False:
            flags |= L.BUILD_NO_SINGLE_CHAIN
        if bounding_box is None:
            pr = self._params(resolution, None, None, max_points_per_node, flags | L.BUILD_COMPUTE_BBOX)
        else:
            pr = self._params(resolution, bounding_box.min, bounding_box.max, max_points_per_node, flags)
        h = C.c_void_p()
        self._check(self.lib.pcv_build_octree(self.handle, C.byref(pr), C.byref(p), C.byref(h)))
        del keep
        return OctreeResult(self, h)

    def ingest(self, num_points_hint=0, has_intensity=False):
        """Streaming batch ingest (pcv_ingest_begin): the reference's `impl Iterator<Item = PointsBatch>` input of
        build_octree (generation.rs:289-295), one batch at a time in the reference's own AoS layout."""
        h = C.c_void_p()
        self._check(self.lib.pcv_ingest_begin(self.handle, int(num_points_hint), 1 if has_intensity else 0, C.byref(h)))
        return Ingest(self, h, has_intensity)

    def out_of_core(self, resolution, bounding_box, has_intensity=False, max_points_per_pass=0, max_points_per_node=0):
        """Out-of-core build (pcv_ooc_begin): batches of any total size stream through the device into host spills, and
        finish(directory) writes the reference's directory partition by partition. bounding_box is required (the stream is
        read once); max_points_per_pass bounds the points on the device at once (0 = derived from free device memory)."""
        if bounding_box is None:
            raise ValueError("the out-of-core build needs the bounding box up front: the stream is read once")
        pr = self._params(resolution, bounding_box.min, bounding_box.max, max_points_per_node, 0)
        h = C.c_void_p()
        self._check(self.lib.pcv_ooc_begin(self.handle, C.byref(pr), 1 if has_intensity else 0, int(max_points_per_pass), C.byref(h)))
        return OutOfCore(self, h, has_intensity)

    def ooc_bucket_runs(self, resolution, bounding_box, xyz, color, intensity=None, routed=True, octants_only=False):
        """The pass of the out-of-core append on device tensors (pcv_ooc_bucket_runs): xyz (n, 3) f64, color (n, 3) u8,
        intensity (n,) f32 or None. Returns (planes, octant_digits, counts): planes = [cx, cy, cz, oct_rgb] int32 (routed) or
        [x, y, z] f64 + rgb (n, 3) u8 (raw), then intensity; every plane holds the 64 bucket runs one after the other."""
        import torch
        n = int(xyz.shape[0])
        dev = xyz.device
        if routed:
            planes = [torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4)]
        else:
            planes = [torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3)] + [torch.empty((n, 3), dtype=torch.uint8, device=dev)]
        planes.append(torch.empty(n, dtype=torch.float32, device=dev) if intensity is not None else None)
        digits = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        ptrs = (C.c_void_p * 5)(*[None if t is None else t.data_ptr() for t in planes])
        counts = (C.c_uint64 * 64)()
        pr = self._params(resolution, bounding_box.min, bounding_box.max, 0, L.ROUTE_OCTANTS_ONLY if octants_only else 0)
        self.wait_torch()
        self._check(self.lib.pcv_ooc_bucket_runs(self.handle, C.byref(pr), xyz.data_ptr(), color.data_ptr(),
                                                 None if intensity is None else intensity.data_ptr(), n, 1 if routed else 0, ptrs,
                                                 digits.data_ptr(), counts))
        return planes, digits[:n], np.array(counts[:], dtype=np.int64)

    def build_from_ply(self, resolution, filename, with_intensity=False, max_points_per_node=0):
        """build_octree_from_file (generation.rs:272-287) with the decode on the device: the file's vertex records go up as
        they are, a HIP kernel casts x / y / z to f64 and adds the header offset (ply.rs:488-493), the bounding box is
        computed on the device."""
        pr = self._params(resolution, None, None, max_points_per_node, L.BUILD_COMPUTE_BBOX)
        h = C.c_void_p()
        self._check(self.lib.pcv_build_octree_from_ply(self.handle, C.byref(pr), str(filename).encode(), 1 if with_intensity else 0,
                                                       C.byref(h)))
        return OctreeResult(self, h)

    def build_from_las(self, resolution, filename, max_points_per_node=0, **las):
        """pcv_build_octree_from_las: las_load and the build with the bounding box computed on the device; **las are
        las_params' keywords (keep_intensity=True gives the octree its intensity)."""
        hdr = read_las_header(filename)
        pr = self._params(resolution, None, None, max_points_per_node, L.BUILD_COMPUTE_BBOX)
        lp, keep = las_params(hdr, **las)
        h = C.c_void_p()
        self._check(self.lib.pcv_build_octree_from_las(self.handle, C.byref(pr), os.fsencode(str(filename)), C.byref(lp), C.byref(h)))
        del keep
        return OctreeResult(self, h)

    def las_load(self, path, **las):
        """A LAS file decoded and filtered on the device (pcv_las_load) -> LasCloud. **las: las_params' keywords."""
        hdr = read_las_header(path)
        lp, keep = las_params(hdr, **las)
        h = C.c_void_p()
        self._check(self.lib.pcv_las_load(self.handle, os.fsencode(str(path)), C.byref(lp), C.byref(h)))
        del keep
        return LasCloud(self, h)

    def las_decode(self, header, raw, n=None, **las):
        """The stage entry (pcv_las_decode): n raw records (numpy uint8, or a torch device tensor of bytes) under `header` (a
        LasHeader or read_las_header's dict) -> read_las's dict, as numpy arrays; the kernels run in either case."""
        hdr = _las_header(header)
        lp, keep = las_params(hdr, **las)
        device = _is_torch(raw)
        b = _Buf(raw, np.uint8, "raw")
        if device and not b.device:
            raise ValueError("raw: a torch tensor must live on the device")
        n = b.size // max(1, hdr.record_length) if n is None else int(n)
        if n * hdr.record_length > b.size:
            raise ValueError(f"raw holds {b.size} bytes, {n} records of {hdr.record_length} take more")
        if device:
            self.wait_torch()
        ids = [e.decode() for e in lp.extras[:lp.num_extras]]
        cols, out, bufs = L.LasColumns(), {}, {}

        def column(name, count, dtype):
            if device:
                import torch
                t = torch.empty(max(1, count * np.dtype(dtype).itemsize), dtype=torch.uint8, device=raw.device)
                bufs[name] = (t, count, dtype)
                return t.data_ptr()
            bufs[name] = np.zeros(max(1, count), dtype=dtype)
            return bufs[name].ctypes.data

        cols.x, cols.y, cols.z = column("x", n, np.float64), column("y", n, np.float64), column("z", n, np.float64)
        cols.color = column("color", 3 * n, np.uint8)
        if lp.keep_intensity:
            cols.intensity = column("intensity", n, np.float32)
        for k, name in enumerate(ids):
            cols.extras[k] = column("@" + name, n, _LAS_EXTRA_DTYPES[name])
        info = L.LasInfo()
        self._check(self.lib.pcv_las_decode(self.handle, C.byref(hdr), C.byref(lp), b.ptr, n, L.MEM_DEVICE if device else L.MEM_HOST,
                                            C.byref(cols), C.byref(info)))
        del keep
        m = int(info.num_kept)

        def fetch(name, count):
            if device:
                t, _, dtype = bufs[name]
                return t.cpu().numpy().view(dtype)[:count].copy()
            return bufs[name][:count]

        out = dict(x=fetch("x", m), y=fetch("y", m), z=fetch("z", m), color=fetch("color", 3 * m).reshape(-1, 3),
                   intensity=fetch("intensity", m) if lp.keep_intensity else None,
                   attributes={name: fetch("@" + name, m) for name in ids}, info=_las_info(info))
        return out

    # ---- loading + queries -----------------------------------------------------------------------
    def open_dir(self, directory):
        """Octree::from_data_provider over a directory (octree/mod.rs:156-215)."""
        h = C.c_void_p()
        self._check(self.lib.pcv_octree_open_dir(self.handle, str(directory).encode(), C.byref(h)))
        return OctreeResult(self, h)

    def xray_tiles(self, trees, tile_size_px=256, pixel_size_m=None, strategy="xray", query_from_global=None, intensity_interval=None,
                   background="white", root_node_id="r", max_workspace_bytes=None, min_intensity=0.0, max_intensity=1.0,
                   binning=None, filter_intervals=None):
        """OctreeResult.xray_tiles (same keywords) over several octrees of this context, as build_xray_quadtree with several
        point_cloud_locations (pcv_xray_run_many, or pcv_xray_run_ex with colored_with_intensity or binning): the union of
        their bounding boxes, every tile's points from all of them. `trees` may instead be a list of S2Cloud
        (pcv_xray_run_s2_ex); a list that mixes the two kinds raises ValueError. With S2 clouds, binning may name any scalar
        attribute of the clouds, and filter_intervals is None or a dict {attribute: (lo, hi)} of closed intervals on scalar
        attributes (--filter-interval), ANDed on every tile; an octree carries only color and intensity. Returns an
        XrayTiles."""
        trees = list(trees)
        if not trees:
            raise ValueError("xray_tiles: no octrees given")
        s2 = [isinstance(t, S2Cloud) for t in trees]
        if any(s2) and not all(s2):
            raise ValueError("xray_tiles: a list of octrees or a list of S2 cell clouds, not a mix of both")
        if all(s2):
            return self._xray_tiles_s2(trees, tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background,
                                       root_node_id, max_workspace_bytes, min_intensity, max_intensity, binning, filter_intervals)
        if filter_intervals:
            raise ValueError("xray_tiles: filter_intervals take S2 cell clouds; an octree carries only color and intensity "
                             "(intensity_interval)")
        p = xray_params(tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background, root_node_id,
                        max_workspace_bytes)
        col = xray_coloring(strategy, min_intensity, max_intensity, binning)
        arr = (C.c_void_p * len(trees))(*[t.handle for t in trees])
        h = C.c_void_p()
        if col is None:
            self._check(self.lib.pcv_xray_run_many(self.handle, arr, len(trees), C.byref(p), C.byref(h)))
        else:
            self._check(self.lib.pcv_xray_run_ex(self.handle, arr, len(trees), C.byref(p), C.byref(col), C.byref(h)))
        return XrayTiles(self, h, int(tile_size_px))

    def _xray_tiles_s2(self, clouds, tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background,
                       root_node_id, max_workspace_bytes, min_intensity, max_intensity, binning, filter_intervals=None):
        for c in clouds:
            c._alive()
        p = xray_params(tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background, root_node_id,
                        max_workspace_bytes)
        col = xray_coloring(strategy, min_intensity, max_intensity, binning)
        arr = (C.c_void_p * len(clouds))(*[c.handle for c in clouds])
        h = C.c_void_p()
        filters, _names = xray_filters(filter_intervals)
        self._check(self.lib.pcv_xray_run_s2_ex(self.handle, arr, len(clouds), C.byref(p), C.byref(col) if col is not None else None,
                                                filters, len(_names), C.byref(h)))
        return XrayTiles(self, h, int(tile_size_px))

    def xray_quadtree(self, trees, tile_size_px=256, pixel_size_m=None, strategy="xray", query_from_global=None,
                      intensity_interval=None, background="white", root_node_id="r", max_workspace_bytes=None, min_intensity=0.0,
                      max_intensity=1.0, binning=None, output_directory=None, png="stored", filter_intervals=None):
        """xray_tiles over several octrees, or several S2 cell clouds (same arguments), with every level above the leaves
        built on the device; with output_directory the quadtree is also written there (XrayTiles.write, PNGs as `png` says)."""
        xt = self.xray_tiles(trees, tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background,
                             root_node_id, max_workspace_bytes, min_intensity, max_intensity, binning, filter_intervals)
        xt.build_parents()
        if output_directory is not None:
            xt.write(output_directory, png=png)
        return xt

    def xray_open(self, directory):
        """Every meta*.pb of an xray quadtree directory as an XrayTiles (pcv_xray_open_dir), in ascending file name order: the
        node list (descending level, then ascending index) and the PNGs, decoded on demand by node_images."""
        return _xray_open(self, directory)

    def xray_merge(self, parts, background="white"):
        """merge_xray_quadtrees over XrayTiles of this context, built (parents built) or opened, mixed (pcv_xray_merge): the
        quadtree with root r, its levels above the parts' roots built on the device over `background`. The result keeps
        its parts alive; freeing one by hand makes its image calls raise PCV_E_INVALID."""
        parts = list(parts)
        arr = (C.c_void_p * max(len(parts), 1))(*[p.handle for p in parts])
        h = C.c_void_p()
        self._check(self.lib.pcv_xray_merge(self.handle, arr, len(parts), _xray_background(background), C.byref(h)))
        xt = XrayTiles(self, h, int(self.lib.pcv_xray_tile_size(h)))
        xt._parts = parts
        return xt

    def shapes(self, shapes):
        """Prepare query shapes on the device. Each entry: ("all",), ("aabb", min3, max3), ("frustum", clip_from_query16),
        ("frustum2", clip_from_query16, query_from_clip16), ("obb", translation3, quat_ijkw4, half_extent3),
        ("web_mercator_rect", north_west2, south_east2) — normalised map coordinates, as web_mercator_rect_from_zoomed
        returns them; the query space is ECEF; ("s2_cells", cell_ids) — PointLocation::S2Cells over an octree: S2 cell ids,
        ascending, of level 1 or finer, taken as given (not normalized); the query space is ECEF (pcv_shapes_create_ex);
        ("polygon", rings, z_min, z_max) — a polygon with holes, or several, under the even-odd rule in the cloud's own x and y,
        times the closed height range (either bound may be infinite; both default to it): `rings` is one (k, 2) array or a list
        of them, each ring implicitly closed; ("polygon_web_mercator", rings) — the same with normalized web-mercator vertices in
        [0, 1) over an ECEF cloud, as polygon_from_lat_lng returns them (pcv_shapes_create_ex2)."""
        arr = (L.Shape * max(1, len(shapes)))()
        unions, polygons = [], []
        for i, sh in enumerate(shapes):
            kind = {"all": L.SHAPE_ALL, "aabb": L.SHAPE_AABB, "frustum": L.SHAPE_FRUSTUM, "obb": L.SHAPE_OBB,
                    "frustum2": L.SHAPE_FRUSTUM_WITH_INVERSE, "web_mercator_rect": L.SHAPE_WEB_MERCATOR_RECT,
                    "s2_cells": L.SHAPE_S2_CELL_UNION, "polygon": L.SHAPE_POLYGON, "polygon_web_mercator": L.SHAPE_POLYGON}[sh[0]]
            arr[i].kind = kind
            if kind == L.SHAPE_S2_CELL_UNION:
                arr[i].reserved = len(unions)
                unions.append(sh[1])
                continue
            if kind == L.SHAPE_POLYGON:
                arr[i].reserved = len(polygons)
                polygons.append(sh[1])
                web = sh[0] == "polygon_web_mercator"
                arr[i].params[0] = float(sh[2]) if not web and len(sh) > 2 else -np.inf
                arr[i].params[1] = float(sh[3]) if not web and len(sh) > 3 else np.inf
                arr[i].params[2] = 1.0 if web else 0.0
                continue
            flat = [float(v) for part in sh[1:] for v in np.asarray(part, dtype=np.float64).ravel()]
            for j, v in enumerate(flat):
                arr[i].params[j] = v
        h = C.c_void_p()
        if polygons:
            first, flat = _s2_unions(unions)
            pfirst, rfirst, verts = _polygon_table(polygons)
            self._check(self.lib.pcv_shapes_create_ex2(self.handle, arr, len(shapes), len(unions), first.ctypes.data, flat.ctypes.data,
                                                       len(polygons), pfirst.ctypes.data, rfirst.ctypes.data, verts.ctypes.data, C.byref(h)))
        elif unions:
            first, flat = _s2_unions(unions)
            self._check(self.lib.pcv_shapes_create_ex(self.handle, arr, len(shapes), len(unions), first.ctypes.data, flat.ctypes.data,
                                                      C.byref(h)))
        else:
            self._check(self.lib.pcv_shapes_create(self.handle, arr, len(shapes), C.byref(h)))
        return Shapes(self, h, len(shapes), [int(arr[i].kind) for i in range(len(shapes))])

    def cull_points(self, shapes, shape_index, x, y, z, intensity=None, interval=None):
        """FilteredIterator keep mask for raw positions. Returns (keep uint8 array/tensor, kept count)."""
        p, keep_alive = self._points(x, y, z, None, intensity)
        iv = (C.c_double * 2)(*[float(v) for v in interval]) if interval is not None else None
        kept = C.c_uint64()
        if p.mem == L.MEM_DEVICE:
            import torch
            keep = torch.empty(p.n, dtype=torch.uint8, device=x.device)
            ptr = keep.data_ptr()
        else:
            keep = np.zeros(p.n, dtype=np.uint8)
            ptr = keep.ctypes.data
        self._check(self.lib.pcv_cull_points(self.handle, shapes.handle, shape_index, C.byref(p), iv, ptr, C.byref(kept)))
        return keep, kept.value

    def transform_points(self, iso7, x, y, z):
        """Isometry3 * Point3 for a batch; iso7 = translation xyz + unit quaternion ijkw."""
        p, keep_alive = self._points(x, y, z)
        iso = (C.c_double * 7)(*[float(v) for v in iso7])
        if p.mem == L.MEM_DEVICE:
            import torch
            out = [torch.empty(p.n, dtype=torch.float64, device=x.device) for _ in range(3)]
            ptrs = [o.data_ptr() for o in out]
        else:
            out = [np.zeros(p.n) for _ in range(3)]
            ptrs = [o.ctypes.data for o in out]
        self._check(self.lib.pcv_transform_points(self.handle, iso, C.byref(p), *ptrs))
        return out

    # ---- S2 cell clouds --------------------------------------------------------------
    def s2_cell_ids(self, x, y, z, level=30):
        """pcv_s2_cell_ids: CellID::from_point(p).parent(level) per point on the device, as uint64 (numpy for host
        inputs; for device tensors an int64 tensor holding the same 64 bits)."""
        p, keep_alive = self._points(x, y, z)
        if p.mem == L.MEM_DEVICE:
            import torch
            ids = torch.empty(p.n, dtype=torch.int64, device=x.device)
            self._check(self.lib.pcv_s2_cell_ids(self.handle, C.byref(p), int(level), ids.data_ptr(), L.MEM_DEVICE))
            return ids
        ids = np.zeros(p.n, dtype=np.uint64)
        self._check(self.lib.pcv_s2_cell_ids(self.handle, C.byref(p), int(level), ids.ctypes.data, L.MEM_HOST))
        return ids

    def s2_union_contains(self, cells, x, y, z):
        """pcv_s2_union_contains: CellUnion::contains per point for `cells`, cell ids ascending; uint8 flags that live
        where the points live."""
        cells = np.ascontiguousarray(cells, dtype=np.uint64).ravel()
        p, keep_alive = self._points(x, y, z)
        if p.mem == L.MEM_DEVICE:
            import torch
            keep = torch.empty(p.n, dtype=torch.uint8, device=x.device)
            ptr = keep.data_ptr()
        else:
            keep = np.zeros(p.n, dtype=np.uint8)
            ptr = keep.ctypes.data
        self._check(self.lib.pcv_s2_union_contains(self.handle, cells.ctypes.data, cells.size, C.byref(p), ptr, p.mem))
        return keep

    def s2_split(self, points, split_level=20):
        """S2Splitter::write for one batch: `points` = dict(x=, y=, z=, color=[, intensity=][, attributes=]) of ECEF points
        (host arrays or device tensors) grouped by their S2 cell at split_level -> S2Cloud. attributes: a dict from name to
        column — (n,) of a scalar dtype, (n, 3) u8 or (n, 3) f64; `(tensor, "u64")` states the type where the dtype cannot
        (pcv_s2_split_ex). An invalid ECEF point raises PcvError (PCV_E_INVALID) naming the first one."""
        p, keep_alive = self._points(points["x"], points["y"], points["z"], points["color"], points.get("intensity"))
        attrs, num_attrs, keep_attrs = _attributes(points.get("attributes"), p.n, p.mem == L.MEM_DEVICE)
        h = C.c_void_p()
        if num_attrs:
            self._check(self.lib.pcv_s2_split_ex(self.handle, C.byref(p), attrs, num_attrs, int(split_level), C.byref(h)))
        else:
            self._check(self.lib.pcv_s2_split(self.handle, C.byref(p), int(split_level), C.byref(h)))
        return S2Cloud(self, h)

    def s2_open(self, directory):
        """S2Cells::from_data_provider over a directory (pcv_s2_open_dir): the S2Cloud that s2_split makes, its cell files read
        and uploaded on first use. PcvError carries the reference's messages for a meta.pb that is too old or not S2."""
        h = C.c_void_p()
        self._check(self.lib.pcv_s2_open_dir(self.handle, os.fsencode(str(directory)), C.byref(h)))
        return S2Cloud(self, h)

    def s2_stream(self, split_level=20, directory=None, open_mode="truncate", flush_points=None):
        """S2Splitter over a stream of batches (pcv_s2_stream_*) -> S2Stream. directory None: the cloud is merged on the
        device at finish() and equals s2_split of the concatenated batches. With a directory the cells' files are written as
        the stream goes (a flush whenever flush_points points are pending, None = the library's default), the total is
        unbounded, and finish() returns the cloud that s2_open opens. open_mode "append" (OpenMode::Append) adds to the S2
        directory that is there: no file is truncated, meta.pb counts the old points and the new."""
        modes = {"truncate": L.S2_TRUNCATE, "append": L.S2_APPEND}
        if open_mode not in modes:
            raise ValueError('open_mode must be "truncate" or "append"')
        pr = L.S2StreamParams()
        pr.struct_size = C.sizeof(L.S2StreamParams)
        if not 0 <= int(split_level) <= 0xFFFFFFFF:
            raise L.PcvError(L.PCV_E_INVALID, "an S2 split level is 0 ..= 30")
        pr.split_level = int(split_level)
        pr.directory = os.fsencode(str(directory)) if directory is not None else None
        pr.open_mode = modes[open_mode]
        pr.flush_points = int(flush_points or 0)
        h = C.c_void_p()
        self._check(self.lib.pcv_s2_stream_begin(self.handle, C.byref(pr), C.byref(h)))
        return S2Stream(self, h)

    # ---- stage-level entry points ----------------------------------------------------------------
    def aabb_reduce(self, x, y, z):
        p, keep = self._points(x, y, z)
        bmin, bmax = (C.c_double * 3)(), (C.c_double * 3)()
        self._check(self.lib.pcv_aabb_reduce(self.handle, C.byref(p), bmin, bmax))
        return np.array(bmin[:]), np.array(bmax[:])

    def chain_keys(self, resolution, bounding_box, x, y, z, nlevels=0):
        p, keep = self._points(x, y, z)
        pr = self._params(resolution, bounding_box.min, bounding_box.max)
        if p.mem == L.MEM_DEVICE:
            import torch
            keys = torch.empty(p.n, dtype=torch.int64, device=x.device)
            self._check(self.lib.pcv_chain_keys(self.handle, C.byref(pr), C.byref(p), nlevels, keys.data_ptr()))
            return keys
        keys = np.zeros(p.n, dtype=np.uint64)
        self._check(self.lib.pcv_chain_keys(self.handle, C.byref(pr), C.byref(p), nlevels, keys.ctypes.data))
        return keys

    def node_split(self, resolution, bounding_box, sorted_keys, max_points_per_node=0, capacity=1 << 16):
        """K4 on sorted full-depth path keys: ctypes array of SplitNode (breadth first, children consecutive)."""
        b = _Buf(sorted_keys, np.uint64, "sorted_keys")
        pr = self._params(resolution, bounding_box.min, bounding_box.max, max_points_per_node)
        nodes = (L.SplitNode * capacity)()
        num = C.c_uint64()
        self._check(self.lib.pcv_node_split(self.handle, C.byref(pr), b.ptr, b.size, L.MEM_DEVICE if b.device else L.MEM_HOST,
                                            nodes, capacity, C.byref(num)))
        if num.value > capacity:
            return self.node_split(resolution, bounding_box, sorted_keys, max_points_per_node, int(num.value))
        return nodes, int(num.value)

    def gather_encode(self, resolution, bounding_box, x, y, z, color, nodes, num_nodes, intensity=None, max_points_per_node=0):
        """K5 + K6 for a given topology (node_split's table): the finished octree."""
        p, keep = self._points(x, y, z, color, intensity)
        pr = self._params(resolution, bounding_box.min, bounding_box.max, max_points_per_node)
        h = C.c_void_p()
        self._check(self.lib.pcv_gather_encode(self.handle, C.byref(pr), C.byref(p), nodes, num_nodes, C.byref(h)))
        del keep
        return OctreeResult(self, h)

    def selftest_division(self, divisors, samples_per_divisor=1 << 22):
        """Number of inputs for which the exact constant-divisor division differs from IEEE division (must be 0)."""
        d = np.ascontiguousarray(divisors, dtype=np.float64)
        bad = C.c_uint64()
        self._check(self.lib.pcv_selftest_division(self.handle, d.ctypes.data_as(C.POINTER(C.c_double)), d.size,
                                                   int(samples_per_divisor), C.byref(bad)))
        return bad.value

    def route_buckets(self, resolution, bounding_box, x, y, z, color=None, with_state=False):
        """(bucket int32 tensor, 64 counts[, state]) for device-resident points: bucket = 8 * level-1 digit + level-2
        digit. with_state (needs color) also returns the level-1 chain state dict(cx, cy, cz = Float32 bits of the
        level-1 codes, oct_rgb = digit | r << 8 | g << 16 | b << 24), all int32 tensors."""
        import torch
        p, keep = self._points(x, y, z, color if with_state else None)
        if p.mem != L.MEM_DEVICE:
            raise ValueError("route_buckets needs device tensors")
        pr = self._params(resolution, bounding_box.min, bounding_box.max)
        bucket = torch.empty(p.n, dtype=torch.int32, device=x.device)
        counts = (C.c_uint64 * 64)()
        st, state = None, None
        if with_state:
            state = {k: torch.empty(p.n, dtype=torch.int32, device=x.device) for k in ("cx", "cy", "cz", "oct_rgb")}
            st = L.RouteState(state["cx"].data_ptr(), state["cy"].data_ptr(), state["cz"].data_ptr(), state["oct_rgb"].data_ptr())
        self._check(self.lib.pcv_route_buckets(self.handle, C.byref(pr), C.byref(p), bucket.data_ptr(), counts,
                                               C.byref(st) if st is not None else None))
        counts = np.array(counts[:], dtype=np.int64)
        return (bucket, counts, state) if with_state else (bucket, counts)

    def route_plan(self, resolution, bounding_box, x, y, z, octants_only=False, out=None):
        """First pass of the two-pass routing (pcv_route_plan): (bucket uint8 tensor, per-tile bucket histograms, 64 counts)
        for device-resident points; the histograms are what pcv_route_scatter derives every owner's row offsets from.
        octants_only: ownership by root octant — the bucket is the level-1 digit alone (PCV_ROUTE_OCTANTS_ONLY). out: (bucket,
        tile_hist) tensors of an earlier call with the same number of points, reused."""
        import torch
        p, keep = self._points(x, y, z, None)
        if p.mem != L.MEM_DEVICE:
            raise ValueError("route_plan needs device tensors")
        pr = self._params(resolution, bounding_box.min, bounding_box.max, 0, L.ROUTE_OCTANTS_ONLY if octants_only else 0)
        tiles = int(self.lib.pcv_route_tiles(p.n))
        if out is not None and int(out[0].numel()) == p.n and int(out[1].shape[0]) == max(tiles, 1):
            bucket, tile_hist = out
        else:
            bucket = torch.empty(p.n, dtype=torch.uint8, device=x.device)
            tile_hist = torch.empty((max(tiles, 1), 64), dtype=torch.int16, device=x.device)
        counts = (C.c_uint64 * 64)()
        self._check(self.lib.pcv_route_plan(self.handle, C.byref(pr), C.byref(p), bucket.data_ptr(), tile_hist.data_ptr(), counts))
        return bucket, tile_hist, np.array(counts[:], dtype=np.int64)

    def route_scatter(self, resolution, bounding_box, x, y, z, color, bucket, tile_hist, rank_of_bucket, dsts, intensity=None):
        """Second pass (pcv_route_scatter): the level-1 state of every point written straight to its owner's planes.
        dsts[r] = dict(oct_rgb, cx, cy, cz[, intensity]) of int32 (float32) device tensors (views into send / receive buffers)."""
        p, keep = self._points(x, y, z, color, intensity)
        pr = self._params(resolution, bounding_box.min, bounding_box.max)
        world = len(dsts)
        arr = (L.RouteDst * world)()
        for r, d in enumerate(dsts):
            for k in ("oct_rgb", "cx", "cy", "cz"):
                setattr(arr[r], k, d[k].data_ptr() if d[k].numel() else None)
            arr[r].intensity = d["intensity"].data_ptr() if intensity is not None and d["intensity"].numel() else None
        table = (C.c_uint8 * 64)(*[int(v) for v in rank_of_bucket])
        self._check(self.lib.pcv_route_scatter(self.handle, C.byref(pr), C.byref(p), bucket.data_ptr(), tile_hist.data_ptr(), world,
                                               table, arr))
        del keep

    def partition_by_owner(self, owner, planes, dsts, rank_of_bucket=None):
        """Stable partition of row-aligned device planes by owner. planes: list of tensors with the same number of rows;
        dsts[r][p]: tensor (view into a send / receive buffer) that receives rank r's rows of plane p in input order.
        With rank_of_bucket (64 entries) `owner` holds buckets and the table maps them to ranks."""
        n = int(planes[0].shape[0])
        world, npl = len(dsts), len(planes)
        arr = (L.Plane * npl)()
        for k, t in enumerate(planes):
            if not t.is_contiguous() or int(t.shape[0]) != n:
                raise ValueError("planes must be contiguous and row-aligned")
            arr[k].src = t.data_ptr()
            arr[k].elem_bytes = t.element_size() * (int(t.numel()) // n if n else 1)
        dst = (C.c_void_p * (world * npl))()
        for r, row in enumerate(dsts):
            for k, t in enumerate(row):
                dst[r * npl + k] = t.data_ptr()
        table = (C.c_uint8 * 64)(*[int(v) for v in rank_of_bucket]) if rank_of_bucket is not None else None
        self._check(self.lib.pcv_partition_by_owner(self.handle, n, owner.data_ptr(), world, table, npl, arr, dst))

    def build_begin_routed(self, resolution, bounding_box, state, intensity=None, max_points_per_node=0,
                           force_split_level1=0):
        """build_begin for points that arrive as their level-1 chain state (route_buckets(with_state=True))."""
        rp = L.RoutedPoints()
        rp.n = int(state["oct_rgb"].shape[0])
        rp.cx, rp.cy, rp.cz, rp.oct_rgb = (state[k].data_ptr() for k in ("cx", "cy", "cz", "oct_rgb"))
        rp.intensity = intensity.data_ptr() if intensity is not None else None
        flags = ((int(force_split_level1) & 0xFF) << 8) | (L.BUILD_STAGE_TIMES if self.stage_times else 0)
        pr = self._params(resolution, bounding_box.min, bounding_box.max, max_points_per_node, flags)
        h = C.c_void_p()
        self._check(self.lib.pcv_build_begin_routed(self.handle, C.byref(pr), C.byref(rp), C.byref(h)))
        return PendingBuild(self, h, (state, intensity))

    def build_begin(self, resolution, bounding_box, x, y, z, color, intensity=None, max_points_per_node=0,
                    force_split_level1=0):
        """First half of the two-step build (multi-GPU path): topology + stream lengths. Returns a PendingBuild; the
        input tensors must stay alive until finish()."""
        p, keep = self._points(x, y, z, color, intensity)
        flags = ((int(force_split_level1) & 0xFF) << 8) | (L.BUILD_STAGE_TIMES if self.stage_times else 0)
        pr = self._params(resolution, bounding_box.min, bounding_box.max, max_points_per_node, flags)
        h = C.c_void_p()
        self._check(self.lib.pcv_build_begin(self.handle, C.byref(pr), C.byref(p), C.byref(h)))
        return PendingBuild(self, h, keep)

    def sort_keys64(self, keys, begin_bit=0, end_bit=64):
        b = _Buf(keys, np.uint64, "keys")
        self._check(self.lib.pcv_sort_keys64(self.handle, b.ptr, b.size, begin_bit, end_bit,
                                             L.MEM_DEVICE if b.device else L.MEM_HOST))
        return b.keep

    def sort_keys32(self, keys, begin_bit=0, end_bit=32):
        b = _Buf(keys, np.uint32, "keys")
        self._check(self.lib.pcv_sort_keys32(self.handle, b.ptr, b.size, begin_bit, end_bit,
                                             L.MEM_DEVICE if b.device else L.MEM_HOST))
        return b.keep

    def sort_pairs32(self, keys, values, begin_bit=0, end_bit=32):
        k, v = _Buf(keys, np.uint32, "keys"), _Buf(values, np.uint32, "values")
        if k.size != v.size:
            raise ValueError("keys and values must have the same length")
        self._check(self.lib.pcv_sort_pairs32(self.handle, k.ptr, v.ptr, k.size, begin_bit, end_bit,
                                              L.MEM_DEVICE if k.device else L.MEM_HOST))
        return k.keep, v.keep

    def sort_records(self, keys, key_bits, vec=None, planes=(), plane0_in=None, color_in=None, color_stride=3, map=None, rows=None,
                     hold_second=False, check_keys=True, packed=False):
        """The build's stable record sort on its own (pcv_sort_records), in place: u32 keys, a payload `vec` of shape (n, 2) (12-byte
        records: the rank sits above a colour byte) or (n, 4) words or none, and up to 8 planes of words; all numpy arrays or all
        device tensors. plane0_in: plane 0 is read from this array, which is left as it is (planes[0] receives the sorted plane).
        rows: None, "device" (counted on the device and returned) or the rank counts per sort workgroup, shape (groups, len(map)).
        packed: `vec` holds the chain pass's 8-byte records (second word: third code | predicted rank << 16) and `keys` only
        receives the sorted keys; on input its first 2 n bytes hold the ranks as half words, which rows="device" counts.
        Returns (keys, vec, planes, rows, plan): the sorted arrays, the rows the device counted (or None) and the plan the sort
        ran as a dict (the fields of pcv_sort_plan_info)."""
        k = _Buf(keys, np.uint32, "keys")
        v = _Buf(vec, np.uint32, "vec")
        pls = [_Buf(p, np.uint32, "plane") for p in planes]
        p0, m = _Buf(plane0_in, np.uint32, "plane0_in"), _Buf(map, np.uint32, "map")
        col = _Buf(color_in, np.uint8, "color_in")
        counted = isinstance(rows, str)
        if counted and rows != "device":
            raise ValueError('rows: None, "device" or an array')
        a = L.SortRecordsArgs()
        a.n, a.key_bits, a.nwords = k.size, key_bits, len(pls)
        a.vec_bytes = 0 if vec is None else 4 * int(vec.shape[-1]) if len(vec.shape) == 2 else -1
        if len(pls) > 8:
            raise ValueError("at most 8 planes")
        groups, chunk = C.c_int32(), C.c_uint64()
        self.lib.pcv_sort_records_geometry(k.size, C.byref(groups), C.byref(chunk))
        if counted:
            shape = (groups.value, m.size)
            if k.device:
                import torch
                rows = torch.zeros(shape, dtype=torch.int32, device=keys.device)
            else:
                rows = np.zeros(shape, dtype=np.uint32)
        r = _Buf(rows, np.uint32, "rows")
        bufs = [b for b in [k, v, p0, m, col, r] + pls if b.keep is not None]
        if any(b.size != k.size for b in pls + ([p0] if plane0_in is not None else [])) or (vec is not None and v.size * 4 != k.size * a.vec_bytes):
            raise ValueError("payload and planes must have one row per key")
        if any(bool(b.device) != bool(k.device) for b in bufs):
            raise ValueError("all arrays in host memory or all on the device")
        if color_in is not None and col.size != k.size * color_stride:
            raise ValueError("color_in must hold n * color_stride bytes")
        if rows is not None and map is not None and r.size != groups.value * m.size:
            raise ValueError("rows must hold groups x len(map) words")
        a.keys, a.vec, a.plane0_in, a.color_in, a.map, a.rows = k.ptr, v.ptr, p0.ptr, col.ptr, m.ptr, r.ptr
        for w, b in enumerate(pls):
            a.planes[w] = b.ptr
        a.color_stride, a.map_entries = color_stride, m.size
        a.rows_mode = L.SORT_ROWS_NONE if rows is None else L.SORT_ROWS_DEVICE if counted else L.SORT_ROWS_GIVEN
        a.hold_second = 1 if hold_second else 0
        a.mem = L.MEM_DEVICE if k.device else L.MEM_HOST
        a.flags = (L.SORT_RECORDS_CHECK_KEYS if check_keys else 0) | (L.SORT_RECORDS_PACKED if packed else 0)
        info = L.SortPlanInfo()
        self._check(self.lib.pcv_sort_records(self.handle, C.byref(a), C.byref(info)))
        plan = {f: getattr(info, f) for f, _ in L.SortPlanInfo._fields_ if f != "passes"}
        plan["passes"] = [{f: getattr(info.passes[i], f) for f, _ in L.SortPassInfo._fields_} for i in range(info.npasses)]
        return k.keep, v.keep, [b.keep for b in pls], (r.keep if counted else None), plan


def promote_assign(nodes, num_nodes, n=0, with_slots=False):
    """Closed form of the every-8th promotion on a node table: (stream_len, num_points, child_offset) arrays and, with
    with_slots, (node_of_slot, slot_in_node) for every position of the leaf-sorted order."""
    lib = L.load_library()
    per = (L.PromoteNode * max(1, num_nodes))()
    node_of = np.zeros(n if with_slots else 0, dtype=np.uint32)
    slot_in = np.zeros(n if with_slots else 0, dtype=np.uint32)
    rc = lib.pcv_promote_assign(nodes, num_nodes, per, n, node_of.ctypes.data if with_slots else None,
                                slot_in.ctypes.data if with_slots else None)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "pcv_promote_assign: inconsistent node table")
    stream = np.array([per[i].stream_len for i in range(num_nodes)], dtype=np.int64)
    kept = np.array([per[i].num_points for i in range(num_nodes)], dtype=np.int64)
    off = np.array([per[i].child_offset for i in range(num_nodes)], dtype=np.int64)
    return (stream, kept, off, node_of, slot_in) if with_slots else (stream, kept, off)


def level_table(bbox_min, bbox_max, resolution, cap=64):
    lib = L.load_library()
    bmin = (C.c_double * 3)(*[float(v) for v in bbox_min])
    bmax = (C.c_double * 3)(*[float(v) for v in bbox_max])
    edge = (C.c_double * (cap + 2))()
    enc = (C.c_int32 * (cap + 2))()
    ml = lib.pcv_level_table(bmin, bmax, float(resolution), cap, edge, enc)
    return ml, np.array(edge[:ml + 1]), np.array(enc[:ml + 1], dtype=np.int32)


def level_shortcuts(bbox_min, bbox_max, resolution):
    """(max_level, digit_mode[k], code_threshold[k]): the per-level shortcuts of the single chain pass for this cube
    (pcv_level_shortcuts; host tables, held against exact arithmetic by tests/test_oracle_kats.py)."""
    lib = L.load_library()
    bmin = (C.c_double * 3)(*[float(v) for v in bbox_min])
    bmax = (C.c_double * 3)(*[float(v) for v in bbox_max])
    mode = (C.c_uint32 * (L.MAX_KEY_LEVELS + 2))()
    thr = (C.c_double * (L.MAX_KEY_LEVELS + 2))()
    ml = lib.pcv_level_shortcuts(bmin, bmax, float(resolution), mode, thr)
    return ml, np.array(mode[:], dtype=np.uint32), np.array(thr[:])


class Ingest:
    """One pcv_ingest: batches of `PointsBatch` shape (src/lib.rs:102-107) go to the device as they are — positions (n, 3)
    f64 AoS like Vec<Point3<f64>>, colour (n, 3) u8, intensity (n,) f32 — and `finish` builds the octree."""

    def __init__(self, ctx, handle, has_intensity):
        self.ctx, self.lib, self.handle, self.has_intensity = ctx, ctx.lib, handle, bool(has_intensity)

    def append(self, position, color, intensity=None):
        pos = np.ascontiguousarray(position, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("position must be (n, 3): one Point3<f64> per row")
        n = pos.shape[0]
        col = np.ascontiguousarray(color, dtype=np.uint8)
        if col.shape != (n, 3):
            raise ValueError("color must be (n, 3) u8")
        inten = None
        if self.has_intensity:
            if intensity is None:
                raise ValueError("the ingest was begun with intensity: every batch must carry it")
            inten = np.ascontiguousarray(intensity, dtype=np.float32)
            if inten.shape != (n,):
                raise ValueError("intensity must be (n,) f32")
        if self.handle is None:
            raise ValueError("the ingest is finished")
        self.ctx._check(self.lib.pcv_ingest_append(self.handle, pos.ctypes.data, col.ctypes.data,
                                                   None if inten is None else inten.ctypes.data, n))

    @property
    def num_points(self):
        return int(self.lib.pcv_ingest_num_points(self.handle)) if self.handle is not None else 0

    def bbox(self):
        lo, hi = (C.c_double * 3)(), (C.c_double * 3)()
        self.ctx._check(self.lib.pcv_ingest_bbox(self.handle, lo, hi))
        return np.array(lo[:]), np.array(hi[:])

    def finish(self, resolution, bounding_box=None, max_points_per_node=0, single_chain=None, stage_times=None):
        """pcv_ingest_finish: bounding_box None = the box folded during the ingest (find_bounding_box); consumes the ingest."""
        flags = 0
        if self.ctx.stage_times if stage_times is None else stage_times:
            flags |= L.BUILD_STAGE_TIMES
        if single_chain is True:
            flags |= L.BUILD_FORCE_SINGLE_CHAIN
        elif single_chain is False:
            flags |= L.BUILD_NO_SINGLE_CHAIN
        if bounding_box is None:
            pr = self.ctx._params(resolution, None, None, max_points_per_node, flags | L.BUILD_COMPUTE_BBOX)
        else:
            pr = self.ctx._params(resolution, bounding_box.min, bounding_box.max, max_points_per_node, flags)
        h, mine = C.c_void_p(), self.handle
        self.handle = None  # consumed whatever the call returns
        self.ctx._check(self.lib.pcv_ingest_finish(mine, C.byref(pr), C.byref(h)))
        return OctreeResult(self.ctx, h)

    def abort(self):
        if self.handle is not None:
            self.lib.pcv_ingest_abort(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.abort()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


class OutOfCore:
    """One pcv_ooc: batches of `PointsBatch` shape (positions (n, 3) f64, colour (n, 3) u8, intensity (n,) f32) of a cloud of
    any size; `finish(directory)` writes the reference's directory and returns the build's statistics (a dict) — the tree
    never exists whole, so there is no OctreeResult."""

    def __init__(self, ctx, handle, has_intensity):
        self.ctx, self.lib, self.handle, self.has_intensity = ctx, ctx.lib, handle, bool(has_intensity)

    def append(self, position, color, intensity=None):
        pos = np.ascontiguousarray(position, dtype=np.float64)
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("position must be (n, 3): one Point3<f64> per row")
        n = pos.shape[0]
        col = np.ascontiguousarray(color, dtype=np.uint8)
        if col.shape != (n, 3):
            raise ValueError("color must be (n, 3) u8")
        inten = None
        if self.has_intensity:
            if intensity is None:
                raise ValueError("the build was begun with intensity: every batch must carry it")
            inten = np.ascontiguousarray(intensity, dtype=np.float32)
            if inten.shape != (n,):
                raise ValueError("intensity must be (n,) f32")
        if self.handle is None:
            raise ValueError("the out-of-core build is finished")
        self.ctx._check(self.lib.pcv_ooc_append(self.handle, pos.ctypes.data, col.ctypes.data,
                                                None if inten is None else inten.ctypes.data, n))

    def finish(self, directory):
        """pcv_ooc_finish: plan, the two passes over the partitions, the directory; consumes the handle whatever it returns."""
        if self.handle is None:
            raise ValueError("the out-of-core build is finished")
        st, mine = L.OocStats(), self.handle
        self.handle = None
        self.ctx._check(self.lib.pcv_ooc_finish(mine, str(directory).encode(), C.byref(st)))
        return {name: getattr(st, name) for name, _ in L.OocStats._fields_}

    def abort(self):
        if self.handle is not None:
            self.lib.pcv_ooc_abort(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.abort()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def ooc_plan(counts, max_points_per_node, level1_can_split, max_points_per_pass):
    """pcv_ooc_plan (host only, pure): (partition_of_bucket[64] with -1 for empty buckets, num_partitions, split_mask) from the
    64 global bucket counts; raises PcvError(PCV_E_OOM) naming the bucket when one unit is larger than the budget."""
    cnt = (C.c_uint64 * 64)(*[int(v) for v in counts])
    part, nparts, mask = (C.c_uint32 * 64)(), C.c_uint32(), C.c_uint32()
    err = C.create_string_buffer(256)
    lib = L.load_library()
    rc = lib.pcv_ooc_plan(cnt, int(max_points_per_node), 1 if level1_can_split else 0, int(max_points_per_pass), part,
                          C.byref(nparts), C.byref(mask), err, 256)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, err.value.decode())
    return np.array([-1 if v == 0xFFFFFFFF else int(v) for v in part], dtype=np.int64), int(nparts.value), int(mask.value)


def ooc_top_layout(l1, l2, split_mask):
    """pcv_ooc_top_layout: distributed.top_layout in the library (host only)."""
    a, b = (C.c_uint64 * 8)(*[int(v) for v in l1]), (C.c_uint64 * 64)(*[int(v) for v in l2])
    tl = L.TopLayout()
    rc = L.load_library().pcv_ooc_top_layout(a, b, int(split_mask), C.byref(tl))
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "top streams exceed 32-bit offsets")
    return dict(root_points=int(tl.root_points), l1_stream=[int(v) for v in tl.l1_stream], l1_offset=[int(v) for v in tl.l1_offset],
                l2_offset=[int(v) for v in tl.l2_offset])


class PendingBuild:
    """A tree between pcv_build_begin and pcv_build_finish."""

    def __init__(self, ctx, handle, keep):
        self.ctx, self.handle, self._keep = ctx, handle, keep
        ctx._children.add(self)

    def top_streams(self):
        """(l1[8], l2[64], l1_split_mask): local stream lengths of the level-1 / level-2 nodes (0 = absent)."""
        ts = L.TopStreams()
        self.ctx._check(self.ctx.lib.pcv_build_top_streams(self.handle, C.byref(ts)))
        return np.array(ts.l1[:], dtype=np.int64), np.array(ts.l2[:], dtype=np.int64), int(ts.l1_split_mask)

    def finish(self, layout=None):
        """Second half: encode, record sort, promotion. layout = dict(root_points, l1_stream[8], l1_offset[8],
        l2_offset[64]) with the GLOBAL top-of-tree streams, or None for a self-contained tree."""
        tl = None
        if layout is not None:
            tl = L.TopLayout()
            tl.root_points = int(layout["root_points"])
            for c in range(8):
                tl.l1_stream[c] = int(layout["l1_stream"][c])
                tl.l1_offset[c] = int(layout["l1_offset"][c])
            for b in range(64):
                tl.l2_offset[b] = int(layout["l2_offset"][b])
        h, self.handle = self.handle, None
        rc = self.ctx.lib.pcv_build_finish(h, C.byref(tl) if tl is not None else None)
        self._keep = None
        if rc != L.PCV_OK:
            msg = self.ctx.lib.pcv_last_error(self.ctx.handle)
            self.ctx.lib.pcv_octree_free(h)
            raise L.PcvError(rc, msg.decode() if msg else "")
        return OctreeResult(self.ctx, h)

    def free(self):
        if self.handle is not None and self.ctx.handle is not None:
            self.ctx.lib.pcv_octree_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Shapes:
    """Prepared query shapes (device resident)."""

    def __init__(self, ctx, handle, count, kinds=None):
        self.ctx, self.handle, self.count = ctx, handle, count
        self.kinds = kinds  # PCV_SHAPE_* per shape, as given
        ctx._children.add(self)

    def get(self, i):
        corners, axes = (C.c_double * 24)(), (C.c_double * (3 * L.MAX_SHAPE_AXES))()
        n, valid = C.c_uint32(), C.c_int()
        self.ctx._check(self.ctx.lib.pcv_shapes_get_ex(self.handle, i, corners, axes, L.MAX_SHAPE_AXES, C.byref(n), C.byref(valid)))
        return np.array(corners[:]).reshape(8, 3), np.array(axes[:3 * n.value]).reshape(n.value, 3), bool(valid.value)

    def union(self, i):
        """The cell ids of shape i, an ("s2_cells", ...) entry, as given (pcv_shapes_union)."""
        n = C.c_uint32()
        self.ctx._check(self.ctx.lib.pcv_shapes_union(self.handle, i, 0, None, C.byref(n)))
        cells = np.zeros(n.value, dtype=np.uint64)
        self.ctx._check(self.ctx.lib.pcv_shapes_union(self.handle, i, cells.size, cells.ctypes.data, C.byref(n)))
        return cells

    def polygon(self, i):
        """The rings of shape i, a ("polygon", ...) or ("polygon_web_mercator", ...) entry, as given: a list of (k, 2) arrays
        (pcv_shapes_polygon)."""
        nr, nv = C.c_uint32(), C.c_uint32()
        self.ctx._check(self.ctx.lib.pcv_shapes_polygon(self.handle, i, 0, None, C.byref(nr), 0, None, C.byref(nv)))
        first, verts = np.zeros(nr.value + 1, dtype=np.uint32), np.zeros((nv.value, 2))
        self.ctx._check(self.ctx.lib.pcv_shapes_polygon(self.handle, i, nr.value, first.ctypes.data, C.byref(nr), nv.value, verts.ctypes.data,
                                                        C.byref(nv)))
        return [verts[first[r]:first[r + 1]].copy() for r in range(nr.value)]

    def free(self):
        if self.handle and self.ctx.handle:
            self.ctx.lib.pcv_shapes_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class OctreeResult:
    """A finished octree held by the library: node table + node-contiguous file bytes."""

    def __init__(self, ctx, handle):
        self.ctx = ctx
        self.lib = ctx.lib
        self.handle = handle
        ctx._children.add(self)

    def free(self):
        if self.handle and self.ctx.handle:
            self.lib.pcv_octree_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    @property
    def num_nodes(self):
        return self.lib.pcv_octree_num_nodes(self.handle)

    @property
    def num_points(self):
        return self.lib.pcv_octree_num_points(self.handle)

    def meta(self):
        res = C.c_double()
        bmin, bmax = (C.c_double * 3)(), (C.c_double * 3)()
        ver = C.c_int()
        self.lib.pcv_octree_meta(self.handle, C.byref(res), bmin, bmax, C.byref(ver))
        return dict(resolution=res.value, bbox_min=np.array(bmin[:]), bbox_max=np.array(bmax[:]), version=ver.value)

    def node(self, i):
        info = L.NodeInfo()
        self.ctx._check(self.lib.pcv_octree_node(self.handle, i, C.byref(info)))
        return info

    def node_data(self, i, which):
        ptr, ln = C.c_void_p(), C.c_uint64()
        self.ctx._check(self.lib.pcv_octree_node_data(self.handle, i, which, C.byref(ptr), C.byref(ln)))
        return C.string_at(ptr, ln.value) if ln.value else b""

    def total_gpu_ms(self):
        """GPU time of the build from its first to its last kernel (PCV_STAGE_TOTAL; measured for every build)."""
        ms = (C.c_float * L.NUM_STAGES)()
        self.lib.pcv_octree_stage_ms(self.handle, ms, L.NUM_STAGES)
        return float(ms[L.NUM_STAGES - 1])

    def stage_ms(self):
        ms = (C.c_float * L.NUM_STAGES)()
        n = self.lib.pcv_octree_stage_ms(self.handle, ms, L.NUM_STAGES)
        return {L.STAGE_NAMES[i]: ms[i] for i in range(n)}

    def build_info(self):
        """key_levels, attempts (0 = single-chain build, 1 = exact pipeline, >= 2 something was redone) and the
        single-chain statistics (predicted nodes / leaves, points whose leaf is an unsplit candidate, points whose chain
        was continued from a split candidate's codes, points that replayed the chain from their coordinates);
        record_bytes: bytes per record of the record sort (20, or 12 packed); settled_in_sort: points of the leaves the
        record sort's second pass finished itself."""
        lv, at = C.c_int(), C.c_int()
        self.lib.pcv_octree_build_info(self.handle, C.byref(lv), C.byref(at))
        st = (C.c_uint64 * 4)()
        self.lib.pcv_octree_spec_stats(self.handle, st)
        return dict(key_levels=lv.value, attempts=at.value, single_chain=at.value == 0,
                    record_bytes=int(self.lib.pcv_octree_record_bytes(self.handle)), predicted_nodes=st[0], predicted_leaves=st[1], kept_code_points=st[2], replayed_points=st[3],
                    continued_points=int(self.lib.pcv_octree_spec_continued(self.handle)),
                    wide_pool_entries=int(self.lib.pcv_octree_wide_pool_entries(self.handle)),
                    settled_in_sort=int(self.lib.pcv_octree_settled_in_sort(self.handle)))

    def packed_handover(self):
        """How the chain pass handed its records to the record sort (pcv_octree_packed_handover): 1 = 8-byte records and a plane of
        16-bit ranks, loaded as they are by the sort's first pass; 2 = those, unpacked for a sort that cannot take them; 0 = records
        with their colour (the exact pipeline, an intensity plane, routed input, a predicted tree of more than 65 536 nodes)."""
        return int(self.lib.pcv_octree_packed_handover(self.handle))

    def write_dir(self, directory):
        self.ctx._check(self.lib.pcv_octree_write_dir(self.handle, str(directory).encode()))

    # ---- queries ----
    def node_names(self):
        return [node_name(self.node(i).id_high, self.node(i).id_low) for i in range(self.num_nodes)]

    def cull_nodes(self, shapes, with_sizes=False):
        """Relation matrix [shape][node] (0 In, 1 Cross, 2 Out) and optionally relative_size_on_screen."""
        m, f = self.num_nodes, shapes.count
        rel = np.zeros((f, m), dtype=np.uint8)
        sizes = np.zeros((f, m)) if with_sizes else None
        self.ctx._check(self.lib.pcv_cull_nodes(self.ctx.handle, shapes.handle, self.handle, rel.ctypes.data,
                                                sizes.ctypes.data if with_sizes else None))
        return (rel, sizes) if with_sizes else rel

    def cull_nodes_sparse(self, shapes, capacity, with_sizes=True):
        """Per shape the nodes that are not Out, in node order: (counts[f], node_indices[f][capacity], relation, sizes)."""
        f = shapes.count
        counts = np.zeros(f, dtype=np.uint32)
        idx = np.zeros((f, max(capacity, 1)), dtype=np.uint32)
        rel = np.full((f, max(capacity, 1)), 2, dtype=np.uint8)
        sizes = np.zeros((f, max(capacity, 1))) if with_sizes else None
        self.ctx._check(self.lib.pcv_cull_nodes_sparse(self.ctx.handle, shapes.handle, self.handle, capacity, counts.ctypes.data,
                                                       idx.ctypes.data, rel.ctypes.data, sizes.ctypes.data if with_sizes else None))
        return counts, idx, rel, sizes

    def _traverse(self, fn, shapes, with_status):
        m, f = max(1, self.num_nodes), shapes.count
        counts = np.zeros(f, dtype=np.uint32)
        idx = np.zeros((f, m), dtype=np.uint32)
        status = np.zeros(f, dtype=np.int32)
        if with_status:
            self.ctx._check(fn(self.ctx.handle, shapes.handle, self.handle, m, counts.ctypes.data, idx.ctypes.data,
                               status.ctypes.data))
        else:
            self.ctx._check(fn(self.ctx.handle, shapes.handle, self.handle, m, counts.ctypes.data, idx.ctypes.data))
        return [idx[i, :counts[i]].copy() for i in range(f)], status

    def visible_nodes(self, frusta):
        """Octree::get_visible_nodes per frustum: (list of node-index arrays in heap pop order, status array)."""
        return self._traverse(self.lib.pcv_visible_nodes, frusta, True)

    def nodes_in_location(self, shapes):
        return self._traverse(self.lib.pcv_nodes_in_location, shapes, False)[0]

    def cull_node_points(self, shapes, shape_index, node, interval=None):
        n = self.node(node).num_points
        keep = np.zeros(n, dtype=np.uint8)
        kept = C.c_uint64()
        iv = (C.c_double * 2)(*[float(v) for v in interval]) if interval is not None else None
        self.ctx._check(self.lib.pcv_cull_node_points(self.ctx.handle, shapes.handle, shape_index, self.handle, node, iv,
                                                      keep.ctypes.data, C.byref(kept)))
        return keep, kept.value

    def query_points(self, shapes, shape_index, interval=None, capacity=None, node=None):
        """All points of the octree inside shape `shape_index` (and the intensity interval): dict of numpy arrays
        x, y, z (decoded f64), rgb (n x 3), intensity (or None), in (node traversal, point) order. With `node` only
        that node's points (stream_points_for_query_in_node)."""
        cap = (self.num_points if node is None else self.node(node).num_points) if capacity is None else int(capacity)
        x, y, z = np.zeros(cap), np.zeros(cap), np.zeros(cap)
        rgb = np.zeros((cap, 3), dtype=np.uint8)
        has_int = bool(self.lib.pcv_octree_has_intensity(self.handle))
        inten = np.zeros(cap, dtype=np.float32) if has_int else None
        iv = (C.c_double * 2)(*[float(v) for v in interval]) if interval is not None else None
        count = C.c_uint64()
        outs = (cap, L.MEM_HOST, x.ctypes.data, y.ctypes.data, z.ctypes.data, rgb.ctypes.data,
                inten.ctypes.data if has_int else None, C.byref(count))
        if node is None:
            self.ctx._check(self.lib.pcv_query_points(self.ctx.handle, shapes.handle, shape_index, self.handle, iv, *outs))
        else:
            self.ctx._check(self.lib.pcv_query_node_points(self.ctx.handle, shapes.handle, shape_index, self.handle, int(node),
                                                           iv, *outs))
        n = min(count.value, cap)
        return dict(count=count.value, x=x[:n], y=y[:n], z=z[:n], rgb=rgb[:n], intensity=inten[:n] if has_int else None)

    def query_batch(self, shapes, intervals=None):
        """The points of every shape of `shapes` in one run (pcv_query_batch_run), kept on the device as one segment per
        (shape, node of nodes_in_location). intervals: None, or one entry per shape, None or (lo, hi) on intensity."""
        iv = used = None
        if intervals is not None:
            intervals = list(intervals)
            if len(intervals) != shapes.count:
                raise ValueError(f"intervals: expected {shapes.count} entries (one per shape), got {len(intervals)}")
            iv = (C.c_double * max(1, 2 * shapes.count))()
            used = (C.c_uint8 * max(1, shapes.count))()
            for s, v in enumerate(intervals):
                if v is not None:
                    lo, hi = v
                    iv[2 * s], iv[2 * s + 1], used[s] = float(lo), float(hi), 1
        h = C.c_void_p()
        self.ctx._check(self.lib.pcv_query_batch_run(self.ctx.handle, shapes.handle, self.handle, iv, used, C.byref(h)))
        return QueryBatch(self, h, shapes.count)

    def terrain(self, shapes=None, **params):
        """A finished Terrain of the points `shapes` select (None: all points): one batched query, its segments
        streamed into the grid on the device. params: terrain_params' arguments."""
        return _cloud_terrain(self, shapes, params)

    def map_tiles(self, zoom, min_zoom=None, shapes=None, **params):
        """A finished MapTiles layer of the points `shapes` select (None: all points) of this ECEF octree at
        `zoom`, with the parent levels down to `min_zoom` (None: none); params: map_tiles_params' arguments."""
        return _cloud_map_tiles(self, shapes, zoom, min_zoom, params)

    def xray_tiles(self, tile_size_px=256, pixel_size_m=None, strategy="xray", query_from_global=None, intensity_interval=None,
                   background="white", root_node_id="r", max_workspace_bytes=None, min_intensity=0.0, max_intensity=1.0,
                   binning=None):
        """The leaf level of xray's build_xray_quadtree (xray/src/generation.rs:557-648) rasterised on the device.
        strategy: "xray", "colored", "colored_with_intensity" (IntensityColoringStrategy with min_intensity /
        max_intensity, the reference's defaults 0 and 1) or ("height_stddev", max_stddev, "jet" | "purplish");
        binning: None or ("intensity", bin size), read by colored and colored_with_intensity (pcv_xray_run_ex);
        query_from_global: None or translation xyz + unit quaternion ijkw; intensity_interval: None or (lo, hi); background:
        "white" | "transparent"; root_node_id: a quadtree node name ("r" + base-4 digits). Returns an XrayTiles; its images
        stay on the device."""
        p = xray_params(tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background, root_node_id,
                        max_workspace_bytes)
        col = xray_coloring(strategy, min_intensity, max_intensity, binning)
        h = C.c_void_p()
        if col is None:
            self.ctx._check(self.lib.pcv_xray_run(self.ctx.handle, self.handle, C.byref(p), C.byref(h)))
        else:
            arr = (C.c_void_p * 1)(self.handle)
            self.ctx._check(self.lib.pcv_xray_run_ex(self.ctx.handle, arr, 1, C.byref(p), C.byref(col), C.byref(h)))
        return XrayTiles(self.ctx, h, int(tile_size_px))

    def xray_quadtree(self, tile_size_px=256, pixel_size_m=None, strategy="xray", query_from_global=None, intensity_interval=None,
                      background="white", root_node_id="r", max_workspace_bytes=None, min_intensity=0.0, max_intensity=1.0,
                      binning=None, output_directory=None, png="stored"):
        """xray_tiles (same arguments) with every level above the leaves up to root_node_id built on the device
        (create_non_leaf_nodes, generation.rs:656-682): the whole quadtree; XrayTiles.write puts it on disk, and so does
        this call when output_directory is given (PNGs as `png` says: "stored" or "deflate")."""
        xt = self.xray_tiles(tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background, root_node_id,
                             max_workspace_bytes, min_intensity, max_intensity, binning)
        xt.build_parents()
        if output_directory is not None:
            xt.write(output_directory, png=png)
        return xt

    def render(self, frusta, width, height, point_size=1.0, gamma=1.0, max_nodes=0, depth=False, max_workspace_bytes=None,
               show_octree_nodes=False, outline_color=L.RENDER_OUTLINE_YELLOW, terrain=None, camera_positions=None,
               terrain_window=L.RENDER_TERRAIN_WINDOW):
        """The viewer's frame for every frustum of `frusta` (a Shapes of "frustum" / "frustum2" entries), rasterised on the
        device (pcv_render_views; sdl_viewer/src/lib.rs:158-209): get_visible_nodes, its first max_nodes entries (0: all)
        drawn as points of `point_size` pixels under a depth test, colours through `gamma`, over black. depth=True fetches
        the window-depth planes with the call (they are kept on the device either way). show_octree_nodes (the viewer's `O`
        key, lib.rs:202-208) draws the wireframe of every drawn node's cube right after the node's points, under the same
        depth test, in `outline_color` (r, g, b, a) as given (pcv_render_views_ex). `terrain`: a list of finished Terrains
        or terrain directories, drawn after the nodes as the viewer's wireframe layers (sdl_viewer --terrain; DESIGN §9b
        steps 13-18, pcv_render_views_terrain) in a window of `terrain_window` vertices around each view's camera, whose
        world positions are `camera_positions` [V, 3]. Returns a RenderedViews."""
        p = render_params(width, height, point_size, gamma, max_nodes, max_workspace_bytes)
        h = C.c_void_p()
        if terrain is not None and len(terrain):
            return self._render_terrain(frusta, p, render_overlay(show_octree_nodes, outline_color), list(terrain), camera_positions,
                                        terrain_window, depth)
        if show_octree_nodes:
            o = render_overlay(True, outline_color)
            self.ctx._check(self.lib.pcv_render_views_ex(self.ctx.handle, frusta.handle, self.handle, C.byref(p), C.byref(o), C.byref(h)))
        else:
            self.ctx._check(self.lib.pcv_render_views(self.ctx.handle, frusta.handle, self.handle, C.byref(p), C.byref(h)))
        return RenderedViews(self.ctx, h, frusta.count, int(width), int(height), bool(depth))

    def _render_terrain(self, frusta, p, overlay, terrain, camera_positions, window, depth):
        if camera_positions is None:
            raise L.PcvError(L.PCV_E_INVALID, "render: terrain layers need camera_positions [V, 3]")
        cams = np.ascontiguousarray(camera_positions, dtype=np.float64)
        if cams.shape != (frusta.count, 3):
            raise L.PcvError(L.PCV_E_INVALID, f"camera_positions: expected shape ({frusta.count}, 3), got {cams.shape}")
        opened = []
        try:
            layers = []
            for t in terrain:
                if not isinstance(t, Terrain):
                    t = self.ctx.terrain_open(t)
                    opened.append(t)
                t._live()
                layers.append(t)
            arr = (C.c_void_p * len(layers))(*[t.handle.value if isinstance(t.handle, C.c_void_p) else t.handle for t in layers])
            tl = L.RenderTerrainLayers(len(layers), int(window), arr, cams.ctypes.data)
            h = C.c_void_p()
            self.ctx._check(self.lib.pcv_render_views_terrain(self.ctx.handle, frusta.handle, self.handle, C.byref(p), C.byref(overlay),
                                                              C.byref(tl), C.byref(h)))
        finally:
            for t in opened:
                t.free()
        return RenderedViews(self.ctx, h, frusta.count, int(p.width), int(p.height), bool(depth), len(layers))

    def nodes_blob(self, node_indices):
        """octree_web_viewer's /nodes_data reply body for the given nodes."""
        idx = np.ascontiguousarray(node_indices, dtype=np.uint64)
        need = C.c_uint64()
        ip = idx.ctypes.data_as(C.POINTER(C.c_uint64))
        self.ctx._check(self.lib.pcv_octree_nodes_blob(self.handle, ip, idx.size, None, 0, C.byref(need)))
        buf = np.zeros(need.value, dtype=np.uint8)
        self.ctx._check(self.lib.pcv_octree_nodes_blob(self.handle, ip, idx.size, buf.ctypes.data, buf.size, C.byref(need)))
        return buf.tobytes()

    def tiles3d(self, error_factor=None, transform=None, intensity=False, position_mode="auto", chunk_bytes=None):
        """The plan of this octree as an OGC 3D Tiles 1.0 tileset (pcv_tiles3d_plan): a Tiles3D, whose files are
        packed on the device when they are asked for. The octree must outlive it. Arguments: tiles3d_params'."""
        pr = tiles3d_params(error_factor, transform, intensity, position_mode, chunk_bytes)
        h = C.c_void_p()
        self.ctx._check(self.lib.pcv_tiles3d_plan(self.handle, C.byref(pr), C.byref(h)))
        return Tiles3D(self, h, pr)

    def write_nodes(self, directory, min_level=0):
        """Node files of the nodes at level >= min_level, without meta.pb (multi-GPU output)."""
        self.ctx._check(self.lib.pcv_octree_write_nodes(self.handle, str(directory).encode(), int(min_level)))

    def synchronize(self):
        self.ctx.synchronize()

    def copy_node_into(self, i, which, dst):
        """Copy node i's bytes (0 xyz, 1 rgb, 2 intensity) from the device blob into a uint8 tensor/array view."""
        if hasattr(dst, "data_ptr"):
            ptr, cap, mem = dst.data_ptr(), dst.numel() * dst.element_size(), (L.MEM_DEVICE if dst.is_cuda else L.MEM_HOST)
        else:
            ptr, cap, mem = dst.ctypes.data, dst.nbytes, L.MEM_HOST
        self.ctx._check(self.lib.pcv_octree_copy_node(self.handle, i, which, ptr, cap, mem))

    def copy_nodes_into(self, copies, dst):
        """Batch form of copy_node_into: copies = [(node index, (xyz offset, rgb offset, intensity offset))] with None for
        a file kind to skip; everything lands in the one uint8 tensor / array `dst` (one ABI call)."""
        arr = (L.NodeCopy * max(1, len(copies)))()
        for k, (node, offs) in enumerate(copies):
            arr[k].node = int(node)
            for w in range(3):
                arr[k].dst_offset[w] = 0xFFFFFFFFFFFFFFFF if offs[w] is None else int(offs[w])
        if hasattr(dst, "data_ptr"):
            ptr, cap, mem = dst.data_ptr(), dst.numel() * dst.element_size(), (L.MEM_DEVICE if dst.is_cuda else L.MEM_HOST)
        else:
            ptr, cap, mem = dst.ctypes.data, dst.nbytes, L.MEM_HOST
        self.ctx._check(self.lib.pcv_octree_copy_nodes(self.handle, arr, len(copies), ptr, cap, mem))

    def to_dict(self):
        """{node name: dict(id, num_points, encoding, level, xyz, rgb, intensity)} — same shape the test-side
        oracle wrapper uses, so parity tests are plain dict comparisons."""
        has_int = bool(self.lib.pcv_octree_has_intensity(self.handle))
        out = {}
        for i in range(self.num_nodes):
            nd = self.node(i)
            name = node_name(nd.id_high, nd.id_low)
            out[name] = dict(id=(nd.id_high, nd.id_low), num_points=nd.num_points, encoding=nd.encoding,
                             level=nd.level, xyz=self.node_data(i, 0), rgb=self.node_data(i, 1),
                             intensity=self.node_data(i, 2) if has_int else b"",
                             cube_min=tuple(nd.cube_min), cube_edge=nd.cube_edge)
        return out


class QueryBatch:
    """The result of OctreeResult.query_batch: segment k holds what query_points(shape, node=segment_node[k]) returns.
    Holds its octree: the tree's device blobs are read when points are copied out."""

    _prefix = "pcv_query_batch"  # the entry points' family (S2QueryBatch: pcv_s2_query)

    def _fn(self, name):
        return getattr(self.lib, f"{self._prefix}_{name}")

    def __init__(self, tree, handle, num_shapes):
        self.tree, self.ctx, self.lib, self.handle = tree, tree.ctx, tree.lib, handle
        self.num_shapes = num_shapes
        ns, npt = C.c_uint64(), C.c_uint64()
        self.lib.pcv_query_batch_sizes(handle, C.byref(ns), C.byref(npt))
        self.num_segments, self.num_points = ns.value, npt.value
        self._has_int = bool(self.lib.pcv_octree_has_intensity(tree.handle))
        self._segments = None
        self.ctx._children.add(self)

    def _live(self):
        if not self.handle or not self.ctx.handle:
            raise L.PcvError(L.PCV_E_INVALID, "the query batch was freed")
        if not self.tree.handle:
            raise L.PcvError(L.PCV_E_INVALID, "the query batch's octree was freed")

    def segments(self):
        """(shape_first[S + 1], node[num_segments], offset[num_segments + 1]) as numpy arrays (u64, u32, u64)."""
        self._live()
        if self._segments is None:
            first = np.zeros(self.num_shapes + 1, dtype=np.uint64)
            node = np.zeros(max(1, self.num_segments), dtype=np.uint32)
            off = np.zeros(self.num_segments + 1, dtype=np.uint64)
            self.ctx._check(self._fn("segments")(self.handle, first.ctypes.data, node.ctypes.data, off.ctypes.data))
            self._segments = (first, node[:self.num_segments], off)
        return self._segments

    def points(self, first_segment=0, num_segments=None, out=None):
        """The points of segments [first_segment, first_segment + num_segments) (default: to the end), as query_points
        returns them. out: dict of x, y, z (f64), rgb (u8, 3 per point), optionally intensity — torch device tensors or numpy
        arrays of at least `count` points — filled in place and returned in the result."""
        self._live()
        _, _, off = self.segments()
        first = int(first_segment)
        num = self.num_segments - first if num_segments is None else int(num_segments)
        if not (0 <= first <= self.num_segments and 0 <= num <= self.num_segments - first):
            # the library's own range check (PCV_E_INVALID, nothing written)
            self.ctx._check(self._fn("points")(self.handle, max(first, 0), max(num, 0) or (1 << 63), 0, L.MEM_HOST,
                                                            None, None, None, None, None))
        n = int(off[first + num] - off[first])
        if out is None:
            x, y, z = np.zeros(n), np.zeros(n), np.zeros(n)
            rgb = np.zeros((n, 3), dtype=np.uint8)
            inten = np.zeros(n, dtype=np.float32) if self._has_int else None
            mem, cap = L.MEM_HOST, n
        else:
            x, y, z, rgb, inten = out["x"], out["y"], out["z"], out["rgb"], out.get("intensity")
            bufs = [_Buf(x, np.float64, "x"), _Buf(y, np.float64, "y"), _Buf(z, np.float64, "z"), _Buf(rgb, np.uint8, "rgb")]
            if inten is not None:
                bufs.append(_Buf(inten, np.float32, "intensity"))
            if any(b.keep is not a for b, a in zip(bufs, (x, y, z, rgb, inten))):
                raise TypeError("out: arrays must be contiguous and of the result's dtypes")
            if len({b.device for b in bufs}) != 1:
                raise ValueError("out: all host or all device")
            mem = L.MEM_DEVICE if bufs[0].device else L.MEM_HOST
            cap = min(bufs[0].size, bufs[1].size, bufs[2].size, bufs[3].size // 3, bufs[4].size if inten is not None else bufs[0].size)
        ptr = lambda a: None if a is None else (a.data_ptr() if _is_torch(a) else a.ctypes.data)
        if_int = inten if self._has_int else None
        if mem == L.MEM_DEVICE:
            self.ctx.wait_torch()
        self.ctx._check(self._fn("points")(self.handle, first, num, cap, mem, ptr(x), ptr(y), ptr(z), ptr(rgb), ptr(if_int)))
        return dict(count=n, x=x[:n], y=y[:n], z=z[:n], rgb=rgb[:n] if rgb.ndim == 2 else rgb[:3 * n],
                    intensity=if_int[:n] if if_int is not None else None)

    def shape_points(self, s):
        """Everything shape s selected: its segments, concatenated (== query_points(shapes, s))."""
        first, _, _ = self.segments()
        return self.points(int(first[s]), int(first[s + 1] - first[s]))

    def node_points(self, s, node):
        """Shape s's points in one node of its nodes_in_location list (== query_points(shapes, s, node=node))."""
        first, nodes, _ = self.segments()
        hit = np.flatnonzero(nodes[int(first[s]):int(first[s + 1])] == node)
        if hit.size == 0:
            raise KeyError(f"node {node} is not among shape {s}'s nodes")
        return self.points(int(first[s]) + int(hit[0]), 1)

    # ---- PLY output (pcv_*_ply_rows, pcv_*_write_ply) ----
    def _ply_available(self):
        """The attributes a row can carry: name -> type string."""
        have = {"color": "u8vec3"}
        if self._has_int:
            have["intensity"] = "f32"
        return have

    def _ply_range(self, shape, first_segment, num_segments):
        """(first, num) as the library takes them; a range past the end goes through so that the library refuses it."""
        if shape is not None:
            first, _, _ = self.segments()
            return int(first[shape]), int(first[shape + 1] - first[shape])
        first = int(first_segment)
        num = max(self.num_segments - first, 0) if num_segments is None else int(num_segments)
        return first, num

    def ply_layout(self, attributes=None):
        """The row layout for `attributes` (None: every attribute of the cloud; else exactly the named ones) as ply_layout
        returns it. An unknown name raises PcvError with the library's message."""
        have = self._ply_available()
        names = list(have) if attributes is None else [str(a) for a in attributes]
        return ply_layout([(n, have.get(n)) for n in names])

    def ply_rows(self, shape=None, first_segment=0, num_segments=None, attributes=None, device=False):
        """The points of a segment range (or of shape `shape`) as packed PLY rows, packed on the device
        (pcv_query_batch_ply_rows / pcv_s2_query_ply_rows) -> (uint8 array [rows, stride], layout). device=True: a torch
        tensor on the context's device instead of a numpy array."""
        self._live()
        first, num = self._ply_range(shape, first_segment, num_segments)
        names, count, _keep = _ply_names(attributes)
        stride, rows = C.c_uint32(), C.c_uint64()
        fn = self._fn("ply_rows")
        rc = fn(self.handle, first, num, names, count, 0, L.MEM_HOST, None, C.byref(stride), C.byref(rows))
        if rc != L.PCV_OK and (stride.value == 0 or rows.value == 0):  # anything but "capacity too small"
            self.ctx._check(rc)
        layout = self.ply_layout(attributes)
        n, s = rows.value, stride.value
        if device:
            import torch
            out = torch.empty((n, s), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
            self.ctx.wait_torch()
            ptr, mem = out.data_ptr(), L.MEM_DEVICE
        else:
            out = np.zeros((n, s), dtype=np.uint8)
            ptr, mem = out.ctypes.data, L.MEM_HOST
        if n:
            self.ctx._check(fn(self.handle, first, num, names, count, n * s, mem, ptr, C.byref(stride), C.byref(rows)))
        return out, layout

    def write_ply(self, path, shape=None, first_segment=0, num_segments=None, attributes=None, open_mode="truncate", chunk_points=0):
        """PlyNodeWriter over a segment range (or shape `shape`): a binary little-endian PLY with double positions and the
        attributes ascending by name (pcv_query_batch_write_ply / pcv_s2_query_write_ply). open_mode "truncate" | "append";
        chunk_points: rows per piece of the device-to-file pipeline (0: the default). Returns the rows written; a range
        without points writes no file."""
        self._live()
        if open_mode not in ("truncate", "append"):
            raise ValueError("open_mode: 'truncate' or 'append'")
        first, num = self._ply_range(shape, first_segment, num_segments)
        names, count, _keep = _ply_names(attributes)
        pr = L.PlyWriteParams()
        pr.struct_size = C.sizeof(L.PlyWriteParams)
        pr.open_mode = L.PLY_APPEND if open_mode == "append" else L.PLY_TRUNCATE
        pr.attributes, pr.num_attributes, pr.reserved, pr.chunk_points = names, count, 0, int(chunk_points)
        written = C.c_uint64()
        self.ctx._check(self._fn("write_ply")(self.handle, first, num, os.fsencode(str(path)), C.byref(pr), C.byref(written)))
        return written.value

    def write_ply_per_location(self, pattern, attributes=None, open_mode="truncate", chunk_points=0):
        """One file per shape (location): pattern.format(i) holds shape i's points; shapes without points get no file.
        Returns {i: rows written} for the files that exist afterwards because of this call."""
        out = {}
        for i in range(self.num_shapes):
            n = self.write_ply(pattern.format(i), shape=i, attributes=attributes, open_mode=open_mode, chunk_points=chunk_points)
            if n:
                out[i] = n
        return out

    # ---- LAS output (pcv_*_las_records, pcv_*_write_las) ----
    def las_records(self, shape=None, first_segment=0, num_segments=None, device=False, **las):
        """The points of a segment range (or of shape `shape`) as LAS point data records, quantised and packed on the device
        (pcv_query_batch_las_records / pcv_s2_query_las_records) -> (uint8 array [records, record_length], info dict).
        device=True: a torch tensor on the context's device. **las: las_write_params' keywords."""
        self._live()
        first, num = self._ply_range(shape, first_segment, num_segments)
        pr, _keep = las_write_params(**las)
        length, count, info = C.c_uint32(), C.c_uint64(), L.LasWriteInfo()
        fn = self._fn("las_records")
        rc = fn(self.handle, first, num, C.byref(pr), 0, L.MEM_HOST, None, C.byref(length), C.byref(count), C.byref(info))
        if rc != L.PCV_OK and (length.value == 0 or count.value == 0):  # anything but "capacity too small"
            self.ctx._check(rc)
        n, s = count.value, length.value
        if device:
            import torch
            out = torch.empty((n, s), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
            self.ctx.wait_torch()
            ptr, mem = out.data_ptr(), L.MEM_DEVICE
        else:
            out = np.zeros((n, s), dtype=np.uint8)
            ptr, mem = out.ctypes.data, L.MEM_HOST
        if n:
            self.ctx._check(fn(self.handle, first, num, C.byref(pr), n * s, mem, ptr, C.byref(length), C.byref(count), C.byref(info)))
        return out, _las_write_info(info)

    def write_las(self, path, shape=None, first_segment=0, num_segments=None, **las):
        """A LAS 1.2 / 1.4 file of a segment range (or shape `shape`), the records packed on the device
        (pcv_query_batch_write_las / pcv_s2_query_write_las). **las: las_write_params' keywords, open_mode "truncate" | "append"
        and chunk_points among them. Returns the info dict of the records written; a range without points writes no file."""
        self._live()
        first, num = self._ply_range(shape, first_segment, num_segments)
        pr, _keep = las_write_params(**las)
        info = L.LasWriteInfo()
        self.ctx._check(self._fn("write_las")(self.handle, first, num, os.fsencode(str(path)), C.byref(pr), C.byref(info)))
        return _las_write_info(info)

    def write_las_per_location(self, pattern, **las):
        """One file per shape (location): pattern.format(i) holds shape i's points; shapes without points get no file.
        Returns {i: info} for the files that exist afterwards because of this call."""
        out = {}
        for i in range(self.num_shapes):
            info = self.write_las(pattern.format(i), shape=i, **las)
            if info["num_records"]:
                out[i] = info
        return out

    def terrain(self, shape=None, bbox_min=None, bbox_max=None, **params):
        """A finished Terrain of this result's points (of shape `shape`, or of all of them): terrain_params' arguments; the
        box defaults to the cloud's."""
        self._live()
        if bbox_min is None or bbox_max is None:
            bbox_min, bbox_max = _cloud_bbox(self.tree)
        t = self.ctx.terrain_begin(bbox_min, bbox_max, **params)
        try:
            t.add(self, shape=shape)
            return t.finish()
        except Exception:
            t.free()
            raise

    def map_tiles(self, zoom, min_zoom=None, shape=None, **params):
        """A finished MapTiles layer of this result's points (of shape `shape`, or of all of them) at `zoom`, with the
        parent levels down to `min_zoom` (None: none); params: map_tiles_params' arguments."""
        self._live()
        m = self.ctx.map_tiles_begin(zoom, **params)
        try:
            m.add_query_batch(self, shape=shape)
            m.finish()
            return m if min_zoom is None else m.build_parents(min_zoom)
        except Exception:
            m.free()
            raise

    def free(self):
        if self.handle and self.ctx.handle:
            self._fn("free")(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def xray_params(tile_size_px=256, pixel_size_m=None, strategy="xray", query_from_global=None, intensity_interval=None,
                background="white", root_node_id="r", max_workspace_bytes=None):
    """The pcv_xray_params of OctreeResult.xray_tiles (same arguments); unknown names raise ValueError."""
    if pixel_size_m is None:
        raise ValueError("pixel_size_m is required")
    p = L.XrayParams()
    p.tile_size_px, p.pixel_size_m = int(tile_size_px), float(pixel_size_m)
    if isinstance(strategy, str):
        kinds = {"xray": L.XRAY_XRAY, "colored": L.XRAY_COLORED, "colored_with_intensity": L.XRAY_COLORED_WITH_INTENSITY}
        if strategy not in kinds:
            raise ValueError(f"unknown strategy {strategy!r}")
        p.strategy = kinds[strategy]
    else:
        kind, max_stddev, cmap = strategy
        if kind != "height_stddev" or cmap not in ("jet", "purplish"):
            raise ValueError(f"unknown strategy {strategy!r}")
        p.strategy, p.max_stddev = L.XRAY_HEIGHT_STDDEV, float(max_stddev)
        p.colormap = L.XRAY_JET if cmap == "jet" else L.XRAY_PURPLISH
    if background not in ("white", "transparent"):
        raise ValueError(f"unknown background {background!r}")
    p.background = L.XRAY_BG_WHITE if background == "white" else L.XRAY_BG_TRANSPARENT
    p.root_level, p.root_index = quadtree_node_id(root_node_id)
    if query_from_global is not None:
        p.has_query_from_global = 1
        for i, v in enumerate(query_from_global):
            p.query_from_global[i] = float(v)
    if intensity_interval is not None:
        p.interval_attribute = b"intensity"
        p.interval[0], p.interval[1] = float(intensity_interval[0]), float(intensity_interval[1])
    p.max_workspace_bytes = int(max_workspace_bytes or 0)
    return p


def xray_coloring(strategy="xray", min_intensity=0.0, max_intensity=1.0, binning=None):
    """The pcv_xray_coloring of pcv_xray_run_ex, or None where pcv_xray_run / _run_many do: strategy
    "colored_with_intensity" or a binning. binning: None or (attribute name, bin size); the library checks the name."""
    if binning is not None:
        if isinstance(binning, (str, bytes)) or len(binning) != 2:
            raise ValueError(f"binning must be (attribute, bin size), not {binning!r}")
        attr, size = binning
        if not isinstance(attr, str):
            raise ValueError(f"binning attribute must be a str, not {attr!r}")
    if strategy != "colored_with_intensity" and binning is None:
        return None
    col = L.XrayColoring()
    col.min_intensity, col.max_intensity = float(min_intensity), float(max_intensity)
    if binning is not None:
        col.binning_attribute, col.bin_size = binning[0].encode(), float(binning[1])
    return col


def xray_filters(filter_intervals):
    """(pcv_xray_filter array or None, the encoded names it points to) of a dict {attribute: (lo, hi)} or None."""
    if not filter_intervals:
        return None, []
    items = list(filter_intervals.items())
    arr, names = (L.XrayFilter * len(items))(), []
    for k, (name, iv) in enumerate(items):
        if not isinstance(name, (str, bytes)):
            raise ValueError(f"filter_intervals: an attribute name must be a str, not {name!r}")
        if isinstance(iv, (str, bytes)) or len(iv) != 2:
            raise ValueError(f"filter_intervals[{name!r}] must be (lo, hi), not {iv!r}")
        names.append(name if isinstance(name, bytes) else name.encode())
        arr[k].attribute, arr[k].lo, arr[k].hi = names[-1], float(iv[0]), float(iv[1])
    return arr, names


def xray_bins(data, bin_size):
    """pcv_xray_bins_host (host only): the bins of xray's --binning for a numpy array of one of the ten scalar attribute
    types — `(value as f64 / bin_size) as i64` as Rust computes it, by the function the device compiles — as int64."""
    data = np.asarray(data)
    codes = {np.dtype(t): c for c, t, comps in L.ATTR_TYPES.values() if comps == 1}
    if data.dtype not in codes:
        raise L.PcvError(L.PCV_E_INVALID, f"xray_bins: dtype {data.dtype} is no scalar attribute type")
    flat = np.ascontiguousarray(data).ravel()
    out = np.zeros(flat.size, dtype=np.int64)
    _host_check(L.load_library().pcv_xray_bins_host(codes[data.dtype], flat.size, flat.ctypes.data, float(bin_size), out.ctypes.data),
                "pcv_xray_bins_host")
    return out.reshape(data.shape)


def xray_check_attrs(params, clouds, coloring=None, filter_intervals=None):
    """pcv_xray_check_attrs_host (host only): raises PcvError for what the S2 forms of xray_tiles would refuse before any
    device work. clouds: one (attributes, has_intensity) per cloud, attributes a dict name -> type string of
    S2Cloud.attributes (or a proto enum value). filter_intervals: None, a dict {name: (lo, hi)}, or a list of
    (name, lo, hi) whose name may be None or repeat (what the C entry can be handed)."""
    clouds = list(clouds)
    first, names, types = [0], [], []
    for attrs, _ in clouds:
        for name, typ in attrs.items():
            names.append(name if isinstance(name, bytes) else name.encode())
            types.append(typ if isinstance(typ, int) else L.ATTR_TYPES.get(str(typ).lower(), (0,))[0])
        first.append(len(names))
    first = np.asarray(first, dtype=np.uint32)
    types = np.asarray(types, dtype=np.int32)
    has = np.asarray([1 if h else 0 for _, h in clouds], dtype=np.uint8)
    name_arr = (C.c_char_p * max(1, len(names)))(*names)
    if isinstance(filter_intervals, dict) or filter_intervals is None:
        filters, held = xray_filters(filter_intervals)
        nf = len(held)
    else:
        items = list(filter_intervals)
        filters, held, nf = (L.XrayFilter * max(1, len(items)))(), [], len(items)
        for k, (name, lo, hi) in enumerate(items):
            held.append(None if name is None else (name if isinstance(name, bytes) else name.encode()))
            filters[k].attribute, filters[k].lo, filters[k].hi = held[-1], float(lo), float(hi)
    err = C.create_string_buffer(512)
    rc = L.load_library().pcv_xray_check_attrs_host(C.byref(params), C.byref(coloring) if coloring is not None else None, filters, nf,
                                                    len(clouds), first.ctypes.data, name_arr, types.ctypes.data, has.ctypes.data, err, 512)
    if rc != 0:
        raise L.PcvError(rc, err.value.decode())


def xray_check_params(params, tree_has_intensity=True, coloring=None):
    """pcv_xray_check_params (pcv_xray_check_params_ex with a coloring; host only): raises PcvError for what pcv_xray_run
    (pcv_xray_run_ex) would refuse before any device work."""
    err = C.create_string_buffer(256)
    lib = L.load_library()
    if coloring is None:
        rc = lib.pcv_xray_check_params(C.byref(params), int(bool(tree_has_intensity)), err, 256)
    else:
        rc = lib.pcv_xray_check_params_ex(C.byref(params), C.byref(coloring), int(bool(tree_has_intensity)), err, 256)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, err.value.decode())


def quadtree_node_id(name):
    """quadtree NodeId from its Display form ("r" + base-4 digits, quadtree/src/lib.rs:199-234) -> (level, index)."""
    if not name or name[0] != "r" or any(c not in "0123" for c in name[1:]):
        raise ValueError(f"not a quadtree node id: {name!r}")
    return len(name) - 1, (int(name[1:], 4) if len(name) > 1 else 0)


def quadtree_node_name(level, index):
    """NodeId's Display (quadtree/src/lib.rs:218-234): "r" and one base-4 digit per level, most significant first."""
    return "r" + "".join(str((int(index) >> (2 * l)) & 3) for l in range(int(level) - 1, -1, -1))


def xray_leaf_tiles(tile_size_px, pixel_size_m, bbox_min, bbox_max, query_from_global=None, root_node_id="r"):
    """pcv_xray_leaf_tiles (host only): dict(rect=(min x, min y, edge), deepest_level, leaf_index (u64), leaf_ids,
    tile_bbox (n x 6: min xyz, max xyz), query_obb (n x 10, with an isometry; else None))."""
    level, index = quadtree_node_id(root_node_id)
    lib = L.load_library()
    d3 = lambda v: (C.c_double * 3)(*[float(a) for a in v])
    iso = (C.c_double * 7)(*[float(a) for a in query_from_global]) if query_from_global is not None else None
    rect, deepest, n = (C.c_double * 3)(), C.c_uint32(), C.c_uint64()
    err = C.create_string_buffer(256)
    rc = lib.pcv_xray_leaf_tiles(int(tile_size_px), float(pixel_size_m), d3(bbox_min), d3(bbox_max), iso, level, index, 0, rect,
                                 C.byref(deepest), C.byref(n), None, None, None, err, 256)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, err.value.decode())
    cnt = n.value
    idx = np.zeros(max(cnt, 1), dtype=np.uint64)
    boxes = np.zeros((max(cnt, 1), 6))
    obb = np.zeros((max(cnt, 1), 10)) if iso is not None else None
    rc = lib.pcv_xray_leaf_tiles(int(tile_size_px), float(pixel_size_m), d3(bbox_min), d3(bbox_max), iso, level, index, cnt, rect,
                                 C.byref(deepest), C.byref(n), idx.ctypes.data, boxes.ctypes.data,
                                 obb.ctypes.data if obb is not None else None, err, 256)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, err.value.decode())
    return dict(rect=tuple(rect), deepest_level=deepest.value, leaf_index=idx[:cnt],
                leaf_ids=[quadtree_node_name(deepest.value, i) for i in idx[:cnt]], tile_bbox=boxes[:cnt],
                query_obb=obb[:cnt] if obb is not None else None)


def xray_finalize(fn, values):
    """pcv_xray_finalize: the raster kernel's colour functions on the host. fn: "xray" (values = distinct z bucket counts),
    "colored" (n x 4: exact r, g, b sums, count), "jet" / "purplish" (values in [0, 1]), "to_u8" (n x 4 f32 colours),
    "intensity" (n x 3: mean, min, max, each as f32). Returns (n, 4) uint8 RGBA, before any background."""
    fns = {"xray": L.XRAY_FN_XRAY, "colored": L.XRAY_FN_COLORED, "jet": L.XRAY_FN_JET, "purplish": L.XRAY_FN_PURPLISH,
           "to_u8": L.XRAY_FN_TO_U8, "intensity": L.XRAY_FN_INTENSITY}
    v = np.ascontiguousarray(values, dtype=np.float64)
    n = v.shape[0] if v.ndim else 1
    out = np.zeros((n, 4), dtype=np.uint8)
    rc = L.load_library().pcv_xray_finalize(fns[fn], n, v.ctypes.data, out.ctypes.data)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, f"pcv_xray_finalize({fn})")
    return out


def web_mercator_rect_from_zoomed(min_xy, max_xy, z):
    """WebMercatorRect::from_zoomed_coordinates (host only): ("web_mercator_rect", north_west, south_east) for
    Context.shapes, or None where the reference returns None."""
    mn, mx = (C.c_double * 2)(*[float(v) for v in min_xy]), (C.c_double * 2)(*[float(v) for v in max_xy])
    out = (C.c_double * 4)()
    if int(z) < 0 or L.load_library().pcv_wmr_from_zoomed(mn, mx, int(z), out) != L.PCV_OK:
        return None
    return ("web_mercator_rect", np.array(out[0:2]), np.array(out[2:4]))


def _wmr_params(rect):
    if isinstance(rect, tuple) and rect and rect[0] == "web_mercator_rect":
        rect = rect[1:]
    return (C.c_double * 4)(*[float(v) for part in rect for v in np.asarray(part, dtype=np.float64).ravel()])


def _wmr_xyz(x, y, z):
    x, y, z = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y, z))
    if not (x.size == y.size == z.size):
        raise ValueError("x, y, z differ in length")
    return x, y, z


def wmr_corners(rect):
    """pcv_wmr_corners (host only): the (8, 3) ECEF corners of a rectangle's polyhedron, in the reference's order."""
    out = (C.c_double * 24)()
    rc = L.load_library().pcv_wmr_corners(_wmr_params(rect), out)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "pcv_wmr_corners")
    return np.array(out[:]).reshape(8, 3)


def wmr_project(x, y, z):
    """pcv_wmr_project (host only): normalised web-mercator (u, v) of ECEF points, the chain the device runs."""
    x, y, z = _wmr_xyz(x, y, z)
    u, v = np.zeros(x.size), np.zeros(x.size)
    rc = L.load_library().pcv_wmr_project(x.size, x.ctypes.data, y.ctypes.data, z.ctypes.data, u.ctypes.data, v.ctypes.data)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "pcv_wmr_project")
    return u, v


def wmr_contains(rect, x, y, z):
    """pcv_wmr_contains (host only): WebMercatorRect::contains per ECEF point, as uint8 flags."""
    x, y, z = _wmr_xyz(x, y, z)
    keep = np.zeros(x.size, dtype=np.uint8)
    rc = L.load_library().pcv_wmr_contains(_wmr_params(rect), x.size, x.ctypes.data, y.ctypes.data, z.ctypes.data, keep.ctypes.data)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "pcv_wmr_contains")
    return keep


def wmr_from_lat_lng(lat, lng):
    """WebMercatorCoord::from_lat_lng (radians) with the library's own sin / ln: (u, v)."""
    lat, lng = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (lat, lng))
    u, v = np.zeros(lat.size), np.zeros(lat.size)
    rc = L.load_library().pcv_wmr_from_lat_lng(lat.size, lat.ctypes.data, lng.ctypes.data, u.ctypes.data, v.ctypes.data)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "pcv_wmr_from_lat_lng")
    return u, v


def wmr_to_lat_lng(u, v):
    """WebMercatorCoord::to_lat_lng: (latitude, longitude) in radians."""
    u, v = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (u, v))
    lat, lng = np.zeros(u.size), np.zeros(u.size)
    rc = L.load_library().pcv_wmr_to_lat_lng(u.size, u.ctypes.data, v.ctypes.data, lat.ctypes.data, lng.ctypes.data)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "pcv_wmr_to_lat_lng")
    return lat, lng


def wmr_math(fn, a, b=None):
    """pcv_wmr_math (tests): the chain's own atan2(a, b), (sin a, cos a) or ln a."""
    a = np.ascontiguousarray(a, dtype=np.float64).ravel()
    b = np.ascontiguousarray(b, dtype=np.float64).ravel() if b is not None else None
    out, out2 = np.zeros(a.size), np.zeros(a.size)
    rc = L.load_library().pcv_wmr_math(int(fn), a.size, a.ctypes.data, b.ctypes.data if b is not None else None, out.ctypes.data,
                                       out2.ctypes.data)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "pcv_wmr_math")
    return (out, out2) if int(fn) == L.WMR_FN_SINCOS else out


def _xray_background(background):
    if background not in ("white", "transparent"):
        raise ValueError(f"unknown tile background {background!r}")
    return L.XRAY_BG_WHITE if background == "white" else L.XRAY_BG_TRANSPARENT


def _xray_open(ctx, directory):
    lib = L.load_library()
    handle = ctx.handle if ctx is not None else None

    def check(rc):
        if ctx is not None:
            ctx._check(rc)
        elif rc != L.PCV_OK:
            raise L.PcvError(rc, (lib.pcv_host_last_error() or b"").decode(errors="replace"))
    n = C.c_uint32()
    check(lib.pcv_xray_open_dir(handle, os.fsencode(str(directory)), 0, None, C.byref(n)))
    arr = (C.c_void_p * max(n.value, 1))()
    check(lib.pcv_xray_open_dir(handle, os.fsencode(str(directory)), n.value, arr, C.byref(n)))
    return [XrayTiles(ctx, C.c_void_p(arr[i]), int(lib.pcv_xray_tile_size(arr[i]))) for i in range(n.value)]


def xray_open_host(directory):
    """pcv_xray_open_dir without a context (no device): XrayTiles that serve the node list and host images only; they can
    be passed to xray_merge_check and to any context's xray_merge."""
    return _xray_open(None, directory)


def xray_merge_check(parts):
    """pcv_xray_merge_check (host only): (root level L, merged rect (min x, min y, edge)) of merge_xray_quadtrees'
    validate_and_merge_metadata over XrayTiles, or PcvError(PCV_E_INVALID) with the reference's message."""
    lib = L.load_library()
    parts = list(parts)
    arr = (C.c_void_p * max(len(parts), 1))(*[p.handle for p in parts])
    level, rect, err = C.c_uint32(), (C.c_double * 3)(), C.create_string_buffer(256)
    rc = lib.pcv_xray_merge_check(arr, len(parts), C.byref(level), rect, err, 256)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, err.value.decode(errors="replace"))
    return level.value, tuple(rect)


def merge_xray_quadtrees(ctx, input_directories, output_directory, background="white", png="stored"):
    """The reference's merge_xray_quadtrees binary: every partial quadtree of input_directories merged into
    output_directory (which may be one of them); returns the merged XrayTiles. `png` ("stored" or "deflate") applies to
    the levels the merge builds; the parts' files are copied as they are."""
    for d in input_directories:
        if not os.path.exists(d):
            raise FileNotFoundError(f"Input directory {str(d)!r} doesn't exist.")
        if not os.path.isdir(d):
            raise NotADirectoryError(f"{str(d)!r} is not a directory.")
    os.makedirs(output_directory, exist_ok=True)
    parts = [p for d in input_directories for p in ctx.xray_open(d)]
    merged = ctx.xray_merge(parts, background)
    merged.write(output_directory, png=png)
    return merged


def _xray_handles(parts):
    parts = list(parts)
    return parts, (C.c_void_p * max(len(parts), 1))(*[p.handle for p in parts])


def xray_inpaint_check(x, distance_px, neighbors=()):
    """pcv_xray_inpaint_check (host only): raises PcvError(PCV_E_INVALID) with the message of what XrayTiles.inpaint would
    refuse (a white background, a tile size that is no power of two, distance 255, a neighbour that does not fit)."""
    lib = L.load_library()
    nbs, arr = _xray_handles(neighbors)
    err = C.create_string_buffer(512)
    rc = lib.pcv_xray_inpaint_check(x.handle, arr, len(nbs), int(distance_px), err, 512)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, err.value.decode(errors="replace"))


def xray_inpaint_plan(x, neighbors=()):
    """pcv_xray_inpaint_plan (host only): (slots, num_adjacent). slots is a (leaves, 9, 2) uint32 array of (part, node) per
    slot of the stitched image (TopLeft, Top, TopRight, Left, the leaf, Right, BottomLeft, Bottom, BottomRight; part 0 = x,
    k + 1 = neighbors[k]; node = position among that part's leaves), XRAY_INPAINT_ABSENT twice where no tile contributes;
    num_adjacent is the number of neighbour leaves taken."""
    lib = L.load_library()
    nbs, arr = _xray_handles(neighbors)
    n = x.num_created  # the leaves that exist: a built quadtree's created tiles
    slots = np.zeros((max(n, 1), 9, 2), dtype=np.uint32)
    na, err = C.c_uint64(), C.create_string_buffer(512)
    rc = lib.pcv_xray_inpaint_plan(x.handle, arr, len(nbs), n, slots.ctypes.data, C.byref(na), err, 512)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, err.value.decode(errors="replace"))
    return slots[:n], int(na.value)


def inpaint_xray_quadtree(ctx, input_directory, output_directory, inpaint_distance_px, background="white", root_node_id="r",
                          png="stored"):
    """The reference's inpaint_xray_quadtree binary: the (possibly partial) quadtree with root root_node_id of
    input_directory, inpainted with the leaves of the up to four adjacent quadtrees found there, written to
    output_directory (which may be the input). Returns the inpainted XrayTiles. The fill differs from the reference's
    texture synthesis (XrayTiles.inpaint); diagonal quadtrees are never read."""
    level, index = quadtree_node_id(root_node_id)
    parts = ctx.xray_open(input_directory)
    roots = {}
    for p in parts:
        pl, pi = p.nodes()
        if len(pl):
            at = int(np.argmin(pl))
            roots[(int(pl[at]), int(pi[at]))] = p
    if (level, index) not in roots:
        raise FileNotFoundError(f"no quadtree with root {root_node_id!r} in {str(input_directory)!r}")
    x = roots[(level, index)]
    rx, ry = _quadtree_xy(level, index)
    neighbors = []
    for dx, dy in ((-1, 0), (0, 1), (1, 0), (0, -1)):  # Left, Top, Right, Bottom
        nx, ny = rx + dx, ry + dy
        if 0 <= nx < (1 << level) and 0 <= ny < (1 << level) and (level, _quadtree_index(level, nx, ny)) in roots:
            neighbors.append(roots[(level, _quadtree_index(level, nx, ny))])
    if level != 0 and xray_inpaint_plan(x, neighbors)[1] == 0:
        print(f"No adjacent leaf nodes found in neighboring quadtrees. Did you forget to copy them into {str(input_directory)!r}?",
              file=sys.stderr)
    os.makedirs(output_directory, exist_ok=True)
    out = x.inpaint(inpaint_distance_px, background=background, neighbors=neighbors)
    out.write(output_directory, png=png)
    return out


def _quadtree_xy(level, index):
    """SpatialNodeId::from(NodeId) (quadtree/src/lib.rs:314-331)."""
    x = y = 0
    for b in range(level):
        y |= ((index >> (2 * b)) & 1) << b
        x |= ((index >> (2 * b + 1)) & 1) << b
    return x, y


def _quadtree_index(level, x, y):
    index = 0
    for b in range(level):
        index |= ((y >> b) & 1) << (2 * b) | ((x >> b) & 1) << (2 * b + 1)
    return index


def _png_mode(png):
    if png not in ("stored", "deflate"):
        raise ValueError(f"unknown png mode {png!r} (stored or deflate)")
    return L.XRAY_PNG_STORED if png == "stored" else L.XRAY_PNG_DEFLATE


def png_decode(data):
    """pcv_png_decode (host only): the bytes of an RGBA8 PNG file as an (h, w, 4) uint8 array."""
    lib = L.load_library()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    w, h = C.c_uint32(), C.c_uint32()
    rc = lib.pcv_png_decode(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), None, 0)
    if rc == L.PCV_OK:
        out = np.zeros((h.value, w.value, 4), dtype=np.uint8)
        rc = lib.pcv_png_decode(buf.ctypes.data, buf.size, C.byref(w), C.byref(h), out.ctypes.data, out.nbytes)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, (lib.pcv_host_last_error() or b"").decode(errors="replace"))
    return out


def xray_lanczos_taps(tile_size_px):
    """pcv_xray_lanczos_taps (host only): (left (W,) u32, count (W,) u32, weights (W, 12) f32) of the 2:1 resize."""
    W = int(tile_size_px)
    left, count = np.zeros(max(W, 1), dtype=np.uint32), np.zeros(max(W, 1), dtype=np.uint32)
    w = np.zeros((max(W, 1), 12), dtype=np.float32)
    rc = L.load_library().pcv_xray_lanczos_taps(W, left.ctypes.data, count.ctypes.data, w.ctypes.data)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, f"pcv_xray_lanczos_taps({W})")
    return left[:W], count[:W], w[:W]


def xray_png_encode(rgba, png="stored"):
    """pcv_xray_png_encode_ex (host only): an (h, w, 4) uint8 image as PNG bytes; "stored" (filter 0, stored deflate
    blocks: pcv_xray_png_encode) or "deflate" (Sub / Up filters, run-length deflate: the stream of include/pcv_hip.h)."""
    img = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w = int(img.shape[0]), int(img.shape[1])
    lib = L.load_library()
    need = C.c_uint64()
    if png == "stored":
        rc = lib.pcv_xray_png_encode(img.ctypes.data, w, h, None, 0, C.byref(need))
    else:
        rc = lib.pcv_xray_png_encode_ex(img.ctypes.data, w, h, _png_mode(png), None, 0, C.byref(need))
    if rc != L.PCV_OK:
        raise L.PcvError(rc, f"pcv_xray_png_encode({w} x {h})")
    out = np.zeros(need.value, dtype=np.uint8)
    lib.pcv_xray_png_encode_ex(img.ctypes.data, w, h, _png_mode(png), out.ctypes.data, out.nbytes, C.byref(need))
    return out.tobytes()


def _split_files(buf, offsets):
    return [buf[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(len(offsets) - 1)]


def xray_png_encode_tiles(ctx, tiles, chunk_tiles=0):
    """pcv_xray_png_encode_tiles: a (count, W, W, 4) uint8 array through the device encoder of the "deflate" mode; the PNG
    files as a list of bytes. chunk_tiles: tiles per device chunk (0: the context's download chunk)."""
    img = np.ascontiguousarray(tiles, dtype=np.uint8)
    count, w = int(img.shape[0]), int(img.shape[1])
    offsets = np.zeros(count + 1, dtype=np.uint64)
    cap = count * int(ctx.lib.pcv_xray_png_bound(w, w, L.XRAY_PNG_DEFLATE))
    out = np.zeros(max(cap, 1), dtype=np.uint8)
    ctx._check(ctx.lib.pcv_xray_png_encode_tiles(ctx.handle, img.ctypes.data, L.MEM_HOST, w, count, int(chunk_tiles), cap, out.ctypes.data,
                                                 offsets.ctypes.data))
    return _split_files(out, offsets)


def render_params(width, height, point_size=1.0, gamma=1.0, max_nodes=0, max_workspace_bytes=None):
    """The pcv_render_params of OctreeResult.render (same arguments)."""
    p = L.RenderParams()
    p.width, p.height, p.point_size, p.gamma = int(width), int(height), float(point_size), float(gamma)
    p.max_nodes, p.max_workspace_bytes = int(max_nodes), int(max_workspace_bytes or 0)
    return p


def render_check_params(params):
    """pcv_render_check_params (host only): raises PcvError for what pcv_render_views would refuse before any device work."""
    rc = L.load_library().pcv_render_check_params(C.byref(params))
    if rc != L.PCV_OK:
        raise L.PcvError(rc, "pcv_render_check_params")


def render_overlay(show_octree_nodes=False, outline_color=L.RENDER_OUTLINE_YELLOW, flags=None):
    """The pcv_render_overlay of OctreeResult.render; `flags` overrides the flag word (for the checks of the flag word)."""
    color = [int(c) for c in outline_color]
    if len(color) != 4 or not all(0 <= c <= 255 for c in color):
        raise L.PcvError(L.PCV_E_INVALID, "outline_color: four values in 0 ..= 255 (r, g, b, a)")
    o = L.RenderOverlay()
    o.flags = (L.RENDER_OUTLINE_NODES if show_octree_nodes else 0) if flags is None else int(flags)
    o.outline_rgba[:] = color
    return o


def render_check_overlay(overlay):
    """pcv_render_check_overlay (host only): raises PcvError with the library's message for unknown flag bits."""
    msg = C.create_string_buffer(256)
    rc = L.load_library().pcv_render_check_overlay(C.byref(overlay) if overlay is not None else None, msg, 256)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, msg.value.decode())


def render_check_terrain(num_layers, window, layers=True, camera_positions=True):
    """pcv_render_check_terrain_host (host only) over a pcv_render_terrain_layers with `num_layers` entries: `layers` True
    (placeholders that are never read), None (a null array) or a list with None for a null entry; `camera_positions` True or
    None. Raises PcvError with the library's message."""
    n = int(num_layers)
    arr = None
    if layers is not None:
        entries = [1] * n if layers is True else [None if e is None else 1 for e in layers]
        arr = (C.c_void_p * max(len(entries), 1))(*entries)
    cams = (C.c_double * 3)() if camera_positions is not None else None
    tl = L.RenderTerrainLayers(n, int(window), arr, C.cast(cams, C.c_void_p) if cams is not None else None)
    msg = C.create_string_buffer(256)
    rc = L.load_library().pcv_render_check_terrain_host(C.byref(tl), msg, 256)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, msg.value.decode())


def render_terrain_window(params, camera_pos, window=L.RENDER_TERRAIN_WINDOW):
    """The window position (two ints) of a camera at `camera_pos` (world frame) over the grid of `params` (terrain_params or
    its arguments) for a window of `window` vertices (pcv_render_terrain_window_host)."""
    cam = (C.c_double * 3)(*[float(v) for v in camera_pos])
    pos = (C.c_int64 * 2)()
    _host_check(L.load_library().pcv_render_terrain_window_host(C.byref(_terrain_pr(params)), cam, int(window), pos), "pcv_render_terrain_window_host")
    return int(pos[0]), int(pos[1])


def terrain_meta_read(text):
    """meta.json's text through the library's reader (pcv_terrain_meta_read_host): dict(tile_size, world_from_terrain [7],
    origin [3], resolution_m, tiles int32 [n, 2]). Raises PcvError naming the key that is missing or cut off."""
    raw = text.encode() if isinstance(text, str) else bytes(text)
    lib, pr, n = L.load_library(), L.TerrainParams(), C.c_uint64()
    _host_check(lib.pcv_terrain_meta_read_host(raw, len(raw), C.byref(pr), 0, None, C.byref(n)), "pcv_terrain_meta_read_host")
    pos = np.zeros((n.value, 2), dtype=np.int32)
    _host_check(lib.pcv_terrain_meta_read_host(raw, len(raw), C.byref(pr), n.value, pos.ctypes.data, C.byref(n)), "pcv_terrain_meta_read_host")
    return dict(tile_size=int(pr.tile_size), world_from_terrain=np.array(list(pr.world_from_terrain)), origin=np.array(list(pr.origin)),
                resolution_m=float(pr.resolution_m), tiles=pos)


def render_gamma_lut(gamma):
    """pcv_render_gamma_lut (host only): the 256-entry colour table of the frame for `gamma`."""
    lut = np.zeros(256, dtype=np.uint8)
    rc = L.load_library().pcv_render_gamma_lut(float(gamma), lut.ctypes.data)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, f"pcv_render_gamma_lut({gamma})")
    return lut


class RenderedViews:
    """The result of OctreeResult.render: one RGBA8 frame and one window-depth plane per view, on the device."""

    def __init__(self, ctx, handle, num_views, width, height, depth, num_terrain_layers=0):
        self.ctx, self.lib, self.handle = ctx, ctx.lib, handle
        self.num_views, self.width, self.height, self.num_terrain_layers = num_views, width, height, num_terrain_layers
        ctx._children.add(self)
        self._depth = None
        if depth:
            self._depth = self.depth()

    def _alive(self):
        if not self.handle or not self.ctx.handle:
            raise L.PcvError(L.PCV_E_INVALID, "the rendered views were freed")

    def _planes(self, fn, shape_tail, dtype, first, count):
        import torch
        self._alive()
        count = self.num_views - int(first) if count is None else int(count)
        out = torch.empty((max(count, 0), self.height, self.width) + shape_tail, dtype=dtype, device=f"cuda:{self.ctx.device}")
        self.ctx._check(fn(self.handle, int(first), count, out.data_ptr(), L.MEM_DEVICE))
        return out

    def images(self, first=0, count=None):
        """Views [first, first + count) as a torch uint8 tensor [count, H, W, 4] on the context's device; rows top to bottom."""
        import torch
        return self._planes(self.lib.pcv_render_images, (4,), torch.uint8, first, count)

    def depth(self, first=0, count=None):
        """The same views' window depth as a torch float32 tensor [count, H, W] on the device; 1.0 where nothing was drawn."""
        import torch
        if self._depth is not None and first == 0 and count is None:
            return self._depth
        return self._planes(self.lib.pcv_render_depth, (), torch.float32, first, count)

    def info(self, view):
        """dict(status, nodes_visible, nodes_drawn, points_submitted, points_drawn, pixels_covered) of one view."""
        self._alive()
        st, nv, nd = C.c_int32(), C.c_uint32(), C.c_uint32()
        ps, pd, pc = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ctx._check(self.lib.pcv_render_info(self.handle, int(view), C.byref(st), C.byref(nv), C.byref(nd), C.byref(ps),
                                                 C.byref(pd), C.byref(pc)))
        return dict(status=st.value, nodes_visible=nv.value, nodes_drawn=nd.value, points_submitted=ps.value,
                    points_drawn=pd.value, pixels_covered=pc.value)

    def outline_info(self, view):
        """dict(segments_submitted, segments_drawn, outline_pixels) of one view: 12 per drawn node, the segments that survived
        the clip, the pixels of the image an outline won; all zero when the views were rendered without show_octree_nodes."""
        self._alive()
        ss, sd, op = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ctx._check(self.lib.pcv_render_outline_info(self.handle, int(view), C.byref(ss), C.byref(sd), C.byref(op)))
        return dict(segments_submitted=ss.value, segments_drawn=sd.value, outline_pixels=op.value)

    def terrain_info(self, view, layer):
        """dict(pos, edges_submitted, edges_drawn, pixels_won) of one terrain layer in one view: the window position (two
        ints), the edges the mask test draws, those that survived the clip, the pixels of the image the layer won."""
        self._alive()
        pos, es, ed, pw = (C.c_int64 * 2)(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        self.ctx._check(self.lib.pcv_render_terrain_info(self.handle, int(view), int(layer), pos, C.byref(es), C.byref(ed), C.byref(pw)))
        return dict(pos=(int(pos[0]), int(pos[1])), edges_submitted=es.value, edges_drawn=ed.value, pixels_won=pw.value)

    def write_png(self, directory):
        """One view_<index>.png per view (pcv_xray_png_encode's stored-deflate PNG); returns the paths."""
        os.makedirs(str(directory), exist_ok=True)
        paths = []
        for v in range(self.num_views):
            path = os.path.join(str(directory), f"view_{v:05d}.png")
            with open(path, "wb") as f:
                f.write(xray_png_encode(self.images(v, 1)[0].cpu().numpy()))
            paths.append(path)
        return paths

    def close(self):
        if self.handle and self.ctx.handle:
            self.lib.pcv_render_free(self.handle)
        self.handle = None
        self._depth = None

    free = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class XrayTiles:
    """The result of OctreeResult.xray_tiles: the leaf list of the quadtree and the created tiles' RGBA8 images (device)."""

    def __init__(self, ctx, handle, tile_size_px):
        self.ctx, self.lib, self.handle, self.tile_size_px = ctx, (ctx.lib if ctx is not None else L.load_library()), handle, tile_size_px
        self._parts = []  # a merged quadtree keeps its parts alive
        dl, rect, nl, nc = C.c_uint32(), (C.c_double * 3)(), C.c_uint64(), C.c_uint64()
        self.lib.pcv_xray_info(handle, C.byref(dl), rect, C.byref(nl), C.byref(nc))
        self.deepest_level, self.bounding_rect = dl.value, tuple(rect)
        self.leaf_index = np.zeros(max(nl.value, 1), dtype=np.uint64)
        self.created = np.zeros(max(nc.value, 1), dtype=np.uint64)
        self.kept = np.zeros(max(nc.value, 1), dtype=np.uint64)
        self.drawn = np.zeros(max(nc.value, 1), dtype=np.uint64)
        built = self.lib.pcv_xray_tiles(handle, self.leaf_index.ctypes.data, self.created.ctypes.data, self.kept.ctypes.data,
                                        self.drawn.ctypes.data) == L.PCV_OK
        if not built:  # opened or merged (pcv_xray_open_dir, pcv_xray_merge): the leaves are the nodes at deepest_level
            level, index = self.nodes()
            self.leaf_index[:nl.value] = index[level == dl.value]
            self.created[:nc.value] = np.arange(nc.value, dtype=np.uint64)
        self.leaf_index, self.created = self.leaf_index[:nl.value], self.created[:nc.value]
        self.kept, self.drawn = self.kept[:nc.value], self.drawn[:nc.value]
        # colored_with_intensity: kept points with intensity < 0 per created tile (not drawn; 0 for other strategies)
        self.negative = np.zeros(max(nc.value, 1), dtype=np.uint64)
        self.lib.pcv_xray_negative(handle, self.negative.ctypes.data)
        self.negative = self.negative[:nc.value]
        self.leaf_ids = [quadtree_node_name(self.deepest_level, i) for i in self.leaf_index]
        self.created_ids = [self.leaf_ids[int(c)] for c in self.created]
        self.num_created = int(nc.value)
        if ctx is not None:
            ctx._children.add(self)

    def images(self, first=0, count=None, device=False):
        """Created tiles [first, first + count) as a (count, H, W, 4) uint8 array (numpy, or a torch tensor on the
        context's device with device=True); rows top to bottom."""
        self._alive()
        count = self.num_created - int(first) if count is None else int(count)
        W = self.tile_size_px
        if device:
            import torch
            out = torch.empty((max(count, 0), W, W, 4), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
            ptr, cap, mem = out.data_ptr(), out.numel(), L.MEM_DEVICE
        else:
            out = np.zeros((max(count, 0), W, W, 4), dtype=np.uint8)
            ptr, cap, mem = out.ctypes.data, out.nbytes, L.MEM_HOST
        self._check(self.lib.pcv_xray_images(self.handle, int(first), count, cap, mem, ptr))
        return out

    def image(self, i):
        return self.images(i, 1)[0]

    def build_parents(self):
        """Every level above the leaves up to root_node_id (pcv_xray_build_parents); a second call does nothing."""
        self._alive()
        self._check(self.lib.pcv_xray_build_parents(self.handle))

    def nodes(self):
        """(level, index) arrays of Meta.nodes in pcv_xray_nodes' order: created leaves, then parents level by level."""
        self._alive()
        n = C.c_uint64()
        self.lib.pcv_xray_nodes(self.handle, C.byref(n), 0, None, None)
        level, index = np.zeros(max(n.value, 1), dtype=np.uint32), np.zeros(max(n.value, 1), dtype=np.uint64)
        self.lib.pcv_xray_nodes(self.handle, C.byref(n), n.value, level.ctypes.data, index.ctypes.data)
        return level[:n.value], index[:n.value]

    @property
    def node_ids(self):
        """Names of the nodes ("r" + base-4 digits) in node_images' order."""
        level, index = self.nodes()
        return [quadtree_node_name(int(l), int(i)) for l, i in zip(level, index)]

    def node_images(self, first=0, count=None, device=False):
        """Nodes [first, first + count) of node_ids as a (count, W, W, 4) uint8 array (numpy, or a torch tensor on the
        context's device with device=True)."""
        self._alive()
        if count is None:
            n = C.c_uint64()
            self.lib.pcv_xray_nodes(self.handle, C.byref(n), 0, None, None)
            count = n.value - int(first)
        count, W = int(count), self.tile_size_px
        if device:
            import torch
            out = torch.empty((max(count, 0), W, W, 4), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
            ptr, cap, mem = out.data_ptr(), out.numel(), L.MEM_DEVICE
        else:
            out = np.zeros((max(count, 0), W, W, 4), dtype=np.uint8)
            ptr, cap, mem = out.ctypes.data, out.nbytes, L.MEM_HOST
        self._check(self.lib.pcv_xray_node_images(self.handle, int(first), count, cap, mem, ptr))
        return out

    def write(self, directory, png="stored"):
        """build_xray_quadtree's output directory: <node>.png per node and the meta file (pcv_xray_write_dir_ex). png:
        "stored" (the default: filter 0, stored deflate blocks) or "deflate" (compressed on the device; same pixels, same
        file names, same meta file)."""
        self._alive()
        if png == "stored":
            self._check(self.lib.pcv_xray_write_dir(self.handle, os.fsencode(str(directory))))
        else:
            self._check(self.lib.pcv_xray_write_dir_ex(self.handle, os.fsencode(str(directory)), _png_mode(png)))

    def node_pngs(self, first=0, count=None, png="stored"):
        """The complete PNG files of nodes [first, first + count) of node_ids as a list of bytes (pcv_xray_node_pngs): what
        write puts on disk, without a file system. Nodes of opened quadtrees come as their files are."""
        self._alive()
        mode = _png_mode(png)
        if count is None:
            n = C.c_uint64()
            self.lib.pcv_xray_nodes(self.handle, C.byref(n), 0, None, None)
            count = n.value - int(first)
        count = int(count)
        offsets = np.zeros(count + 1, dtype=np.uint64)
        self._check(self.lib.pcv_xray_node_pngs(self.handle, int(first), count, mode, 0, None, offsets.ctypes.data))
        out = np.zeros(max(int(offsets[count]), 1), dtype=np.uint8)
        self._check(self.lib.pcv_xray_node_pngs(self.handle, int(first), count, mode, int(offsets[count]), out.ctypes.data, offsets.ctypes.data))
        return _split_files(out, offsets)

    def inpaint(self, distance_px, background="white", neighbors=(), ctx=None):
        """inpaint_xray_quadtree on the device (pcv_xray_inpaint): the holes of these leaf tiles (transparent background)
        that a close of the alpha mask by distance_px covers are filled, overlapping enlarged tiles blended, the
        background assigned and every parent level rebuilt; neighbors are the up to four quadtrees whose roots are Left,
        Top, Right or Bottom of this one's. Everything but the fill equals the reference byte for byte; the fill is a
        distance-weighted mean of the known pixels, not the reference's texture synthesis. Returns a new XrayTiles that
        owns its images; this one and the neighbors may be freed. ctx: the context, for tiles opened without one."""
        self._alive()
        ctx = ctx if ctx is not None else self.ctx
        if ctx is None:
            raise ValueError("inpaint needs a context (these tiles were opened host only)")
        nbs, arr = _xray_handles(neighbors)
        h = C.c_void_p()
        ctx._check(self.lib.pcv_xray_inpaint(ctx.handle, self.handle, arr, len(nbs), int(distance_px), _xray_background(background),
                                             C.byref(h)))
        return XrayTiles(ctx, h, int(self.lib.pcv_xray_tile_size(h)))

    def inpaint_info(self):
        """pcv_xray_inpaint_info of an inpainted quadtree: per leaf arrays target_pixels, filled_pixels, blended_pixels
        (counted within the final tile) as a dict."""
        self._alive()
        n = self.num_created
        t, f, b = (np.zeros(max(n, 1), dtype=np.uint64) for _ in range(3))
        self._check(self.lib.pcv_xray_inpaint_info(self.handle, t.ctypes.data, f.ctypes.data, b.ctypes.data))
        return {"target_pixels": t[:n], "filled_pixels": f[:n], "blended_pixels": b[:n]}

    def _check(self, rc):
        if self.ctx is not None:
            self.ctx._check(rc)
        elif rc != L.PCV_OK:
            raise L.PcvError(rc, (self.lib.pcv_host_last_error() or b"").decode(errors="replace"))

    def _alive(self):
        if not self.handle or (self.ctx is not None and not self.ctx.handle):
            raise L.PcvError(L.PCV_E_INVALID, "the xray tiles were freed")

    def free(self):
        if self.handle and (self.ctx is None or self.ctx.handle):
            self.lib.pcv_xray_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def write_meta(directory, resolution, bbox_min, bbox_max, nodes):
    """meta.pb (version 13) for a list of (id_high, id_low, num_points, encoding) tuples."""
    lib = L.load_library()
    arr = (L.NodeInfo * max(1, len(nodes)))()
    for k, (hi, lo, npts, enc) in enumerate(nodes):
        arr[k].id_high, arr[k].id_low, arr[k].num_points, arr[k].encoding = int(hi), int(lo), int(npts), int(enc)
    bmin = (C.c_double * 3)(*[float(v) for v in bbox_min])
    bmax = (C.c_double * 3)(*[float(v) for v in bbox_max])
    rc = lib.pcv_write_meta(str(directory).encode(), float(resolution), bmin, bmax, arr, len(nodes))
    if rc != L.PCV_OK:
        raise L.PcvError(rc, f"cannot write meta.pb in {directory}")


def _ply_names(attributes):
    """attributes (None: every attribute of the cloud, else names) as the char** the PLY entry points take ->
    (array or None, count, keep-alive)."""
    if attributes is None:
        return None, 0, []
    keep = [os.fsencode(str(a)) for a in attributes]
    return (C.c_char_p * max(1, len(keep)))(*keep), len(keep), keep


def _ply_columns(attributes):
    """dict name -> type string, or a sequence of (name, type string | None) -> (names char**, types int32[], n, keep-alive). A type
    of None goes down as 0: the library answers "Data type for attribute 'NAME' not found."."""
    items = list(attributes.items()) if isinstance(attributes, dict) else [tuple(a) for a in attributes]
    names = [os.fsencode(str(n)) for n, _ in items]
    codes = []
    for n, t in items:
        if t is not None and str(t).lower() not in L.ATTR_TYPES:
            raise L.PcvError(L.PCV_E_INVALID, f"Attribute data type invalid (attribute '{n}', type {t!r})")
        codes.append(0 if t is None else L.ATTR_TYPES[str(t).lower()][0])
    types = np.array(codes, dtype=np.int32)
    return (C.c_char_p * max(1, len(names)))(*names), types, len(names), (names, types, items)


def ply_layout(attributes):
    """The row of the PLY that write_ply writes for `attributes` — a dict name -> type string ("u8" ... "f64", "u8vec3",
    "f64vec3") or a sequence of (name, type) in any order (pcv_ply_layout_host): dict(stride=bytes per row, names=the attributes
    in row order (ascending by name, bytewise), offsets={name: byte offset}, types={name: type string}, dtype=the packed numpy
    structured dtype of a row, fields named as the header's properties). Position, three doubles, is always at 0."""
    lib = L.load_library()
    names, types, n, keep = _ply_columns(attributes)
    offsets, stride = np.zeros(max(1, n), dtype=np.uint32), C.c_uint32()
    _host_check(lib.pcv_ply_layout_host(names, types.ctypes.data, n, offsets.ctypes.data, C.byref(stride)), "ply_layout")
    items = keep[2]
    order = sorted(range(n), key=lambda k: int(offsets[k]))
    fields = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    for k in order:
        name, typ = str(items[k][0]), str(items[k][1]).lower()
        _, dt, comps = L.ATTR_TYPES[typ]
        if name in ("color", "rgb", "rgba"):
            fields += [(c, dt) for c in ("red", "green", "blue", "alpha")[:comps]]
        elif comps > 1:
            fields += [(f"{name}{i}", dt) for i in range(comps)]
        else:
            fields.append((name, dt))
    try:
        dtype = np.dtype(fields, align=False)
    except ValueError:  # property names that repeat (an attribute `red` beside color): the bytes are what they are, numpy cannot name them
        dtype = None
    return dict(stride=stride.value, names=[str(items[k][0]) for k in order], offsets={str(items[k][0]): int(offsets[k]) for k in range(n)},
                types={str(items[k][0]): str(items[k][1]).lower() for k in range(n)}, dtype=dtype)


def ply_header(attributes, count):
    """The header write_ply writes for `attributes` (as ply_layout takes them) and `count` vertices, as bytes (pcv_ply_header_host)."""
    lib = L.load_library()
    names, types, n, _keep = _ply_columns(attributes)
    need = C.c_uint64()
    _host_check(lib.pcv_ply_header_host(names, types.ctypes.data, n, int(count), None, 0, C.byref(need)), "ply_header")
    buf = C.create_string_buffer(need.value + 1)
    _host_check(lib.pcv_ply_header_host(names, types.ctypes.data, n, int(count), buf, need.value, C.byref(need)), "ply_header")
    return buf.raw[:need.value]


def ply_append_check(path, attributes):
    """What write_ply(open_mode="append") checks before it touches `path` (pcv_ply_append_check_host): the file's vertex count
    (0: no file, or one shorter than the fixed prefix). PcvError: PCV_E_INVALID for a file of other columns or no PLY of this
    writer, PCV_E_IO for one that cannot be read."""
    lib = L.load_library()
    names, types, n, _keep = _ply_columns(attributes)
    old = C.c_uint64()
    _host_check(lib.pcv_ply_append_check_host(os.fsencode(str(path)), names, types.ctypes.data, n, C.byref(old)), "ply_append_check")
    return old.value


_LAS_EXTRA_DTYPES = {"classification": "u1", "classification_flags": "u1", "return_number": "u1", "number_of_returns": "u1",
                     "scan_direction_flag": "u1", "edge_of_flight_line": "u1", "scanner_channel": "u1", "scan_angle": "<f4",
                     "user_data": "u1", "point_source_id": "<u2", "gps_time": "<f8", "nir": "<u2"}


def _las_check(rc):
    if rc != L.PCV_OK:
        raise L.PcvError(rc, L.load_library().pcv_host_last_error().decode())


def _las_header(header):
    if isinstance(header, L.LasHeader):
        return header
    h = L.LasHeader()
    h.version_major, h.version_minor = header["version"]
    h.point_format, h.header_size, h.record_length = header["point_format"], header["header_size"], header["record_length"]
    h.offset_to_points, h.num_points = header["offset_to_points"], header["num_points"]
    for a in range(3):
        h.scale[a], h.offset[a] = header["scale"][a], header["offset"][a]
    return h


def _las_info(info):
    return dict(num_records=int(info.num_records), num_kept=int(info.num_kept), dropped_class=int(info.dropped_class),
                dropped_withheld=int(info.dropped_withheld), max_color=int(info.max_color), max_intensity=int(info.max_intensity),
                color_rule=L.LAS_COLOR_NAMES[info.color_rule], num_pieces=int(info.num_pieces),
                class_hist=np.array(info.class_hist, dtype=np.uint64), return_hist=np.array(info.return_hist, dtype=np.uint64),
                flag_counts=dict(zip(("synthetic", "key_point", "withheld", "overlap"), (int(v) for v in info.flag_counts))))


def read_las_header(path, as_dict=False):
    """The public header block of a LAS 1.0 - 1.4 file (pcv_las_header_host) -> LasHeader, or a dict of its fields."""
    h = L.LasHeader()
    _las_check(L.load_library().pcv_las_header_host(os.fsencode(str(path)), C.byref(h)))
    if not as_dict:
        return h
    return dict(version=(h.version_major, h.version_minor), point_format=h.point_format, header_size=h.header_size,
                record_length=h.record_length, offset_to_points=h.offset_to_points, num_points=int(h.num_points),
                scale=tuple(h.scale), offset=tuple(h.offset))


def las_extras(point_format):
    """The names of the extras a point data record format has, in the order of DESIGN §9j's table."""
    names, count = (C.c_char_p * L.LAS_MAX_EXTRAS)(), C.c_uint32()
    _las_check(L.load_library().pcv_las_extras_host(int(point_format), names, None, C.byref(count)))
    return [names[k].decode() for k in range(count.value)]


def las_params(header, color="auto", classes=None, drop_withheld=False, keep_intensity=False, extras=(), global_from_local=None,
               piece_points=0, check=True):
    """pcv_las_params for a file with `header` -> (LasParams, keep-alive). color: "auto" | "rgb16" | "rgb8" | "intensity" | an
    (r, g, b); classes: the classes to keep (None: all); extras: names, or "all" for every extra the format has;
    global_from_local: translation xyz + unit quaternion ijkw."""
    hdr = _las_header(header)
    p = L.LasParams()
    if isinstance(color, str):
        if color not in L.LAS_COLOR_NAMES[:4]:
            raise ValueError('color is "auto", "rgb16", "rgb8", "intensity" or an (r, g, b)')
        p.color_mode = L.LAS_COLOR_NAMES.index(color)
    else:
        p.color_mode = L.LAS_COLOR_CONSTANT
        for k in range(3):
            p.constant_color[k] = int(color[k])
    for c in (classes if classes is not None else ()):
        if not 0 <= int(c) <= 255:
            raise ValueError("a class is 0 ..= 255")
        p.class_mask[int(c) >> 6] |= 1 << (int(c) & 63)
    if classes is not None and len(list(classes)) == 0:
        raise ValueError("classes: an empty list keeps nothing; pass None to keep every class")
    p.drop_withheld, p.keep_intensity, p.piece_points = int(bool(drop_withheld)), int(bool(keep_intensity)), int(piece_points)
    if global_from_local is not None:
        p.use_transform = 1
        for k in range(7):
            p.global_from_local[k] = float(global_from_local[k])
    names = las_extras(hdr.point_format) if isinstance(extras, str) and extras == "all" else list(extras or ())
    if len(names) > L.LAS_MAX_EXTRAS:
        raise L.PcvError(L.PCV_E_INVALID, f"LAS: more than {L.LAS_MAX_EXTRAS} extras")
    keep = [os.fsencode(n) for n in names]
    for k, b in enumerate(keep):
        p.extras[k] = b
    p.num_extras = len(keep)
    if check:
        _las_check(L.load_library().pcv_las_check_params_host(C.byref(hdr), C.byref(p)))
    return p, keep


def las_decode_host(header, raw, n=None, **las):
    """The host twin of the device decode (pcv_las_decode_host): raw records (bytes or a uint8 array) -> read_las's dict."""
    hdr = _las_header(header)
    lp, keep = las_params(hdr, **las)
    raw = np.frombuffer(raw, dtype=np.uint8) if isinstance(raw, (bytes, bytearray, memoryview)) else np.ascontiguousarray(raw, dtype=np.uint8)
    n = raw.size // max(1, hdr.record_length) if n is None else int(n)
    if n * hdr.record_length > raw.size:
        raise ValueError(f"raw holds {raw.size} bytes, {n} records of {hdr.record_length} take more")
    ids = [e.decode() for e in lp.extras[:lp.num_extras]]
    cols = L.LasColumns()
    arrays = dict(x=np.zeros(max(1, n)), y=np.zeros(max(1, n)), z=np.zeros(max(1, n)), color=np.zeros(max(1, 3 * n), np.uint8),
                  intensity=np.zeros(max(1, n), np.float32))
    ex = {name: np.zeros(max(1, n), _LAS_EXTRA_DTYPES[name]) for name in ids}
    cols.x, cols.y, cols.z = arrays["x"].ctypes.data, arrays["y"].ctypes.data, arrays["z"].ctypes.data
    cols.color, cols.intensity = arrays["color"].ctypes.data, arrays["intensity"].ctypes.data
    for k, name in enumerate(ids):
        cols.extras[k] = ex[name].ctypes.data
    info = L.LasInfo()
    _las_check(L.load_library().pcv_las_decode_host(C.byref(hdr), C.byref(lp), raw.ctypes.data if raw.size else None, n, C.byref(cols),
                                                     C.byref(info)))
    del keep
    m = int(info.num_kept)
    return dict(x=arrays["x"][:m], y=arrays["y"][:m], z=arrays["z"][:m], color=arrays["color"][:3 * m].reshape(-1, 3),
                intensity=arrays["intensity"][:m] if lp.keep_intensity else None, attributes={k: v[:m] for k, v in ex.items()},
                info=_las_info(info))


def read_las(path, extras=(), **las):
    """The one-pass host reader (pcv_las_read): the dict read_ply(extras=True) returns — x, y, z float64, color (n, 3) uint8,
    intensity float32 or None, attributes {name: array} — plus info. **las: las_params' keywords."""
    lib = L.load_library()
    lp, keep = las_params(read_las_header(path), extras=extras, **las)
    h = C.c_void_p()
    _las_check(lib.pcv_las_read(os.fsencode(str(path)), C.byref(lp), C.byref(h)))
    try:
        p = L.Points()
        lib.pcv_las_points(h, C.byref(p))
        n = int(p.n)

        def arr(ptr, dtype, count):
            a = np.zeros(count, dtype=dtype)
            if count:
                C.memmove(a.ctypes.data, ptr, a.nbytes)
            return a

        out = dict(x=arr(p.x, np.float64, n), y=arr(p.y, np.float64, n), z=arr(p.z, np.float64, n),
                   color=arr(p.color, np.uint8, 3 * n).reshape(-1, 3), intensity=arr(p.intensity, np.float32, n) if lp.keep_intensity else None)
        count, attrs = C.c_uint32(), (L.Attribute * L.LAS_MAX_EXTRAS)()
        lib.pcv_las_attributes(h, C.byref(count), attrs)
        out["attributes"] = {os.fsdecode(attrs[k].name): arr(attrs[k].data, _LAS_EXTRA_DTYPES[os.fsdecode(attrs[k].name)], n)
                             for k in range(count.value)}
        info = L.LasInfo()
        lib.pcv_las_info_get(h, C.byref(info))
        out["info"] = _las_info(info)
        return out
    finally:
        lib.pcv_las_free(h)


def las_write_params(point_format="auto", version_minor=0, scale=0.001, offset=None, color="x257", intensity_scale=1.0, fields=None,
                     open_mode="truncate", chunk_points=0, file_source_id=0, global_encoding=0, day=0, year=0, system_identifier="",
                     generating_software=""):
    """pcv_las_write_params -> (LasWriteParams, keep-alive). point_format: 0 - 3, 6 - 8 or "auto"; scale, offset: a
    number or three; offset None: floor(min) per axis of the points written (auto_offset; in append mode the file's offset);
    color: "x257" | "shift8" | "rgb8"; fields: None (every field the source has and the format holds) or names among "color",
    "intensity" and las_extras' names."""
    if open_mode not in ("truncate", "append"):
        raise ValueError("open_mode: 'truncate' or 'append'")
    if color not in L.LAS_WRITE_COLOR_NAMES:
        raise ValueError('color is "x257", "shift8" or "rgb8"')
    p = L.LasWriteParams()
    p.struct_size = C.sizeof(L.LasWriteParams)
    p.open_mode = L.LAS_APPEND if open_mode == "append" else L.LAS_TRUNCATE
    p.point_format = L.LAS_FORMAT_AUTO if isinstance(point_format, str) and point_format == "auto" else int(point_format)
    p.version_minor = int(version_minor)
    three = lambda v: [float(v)] * 3 if np.isscalar(v) else [float(a) for a in v]
    for a, v in enumerate(three(scale)):
        p.scale[a] = v
    p.auto_offset = 1 if offset is None else 0
    if offset is not None:
        for a, v in enumerate(three(offset)):
            p.offset[a] = v
    p.color_rule, p.intensity_scale, p.chunk_points = L.LAS_WRITE_COLOR_NAMES.index(color), float(intensity_scale), int(chunk_points)
    keep = None
    if fields is not None:
        keep = [os.fsencode(str(f)) for f in fields]
        arr = (C.c_char_p * max(1, len(keep)))(*keep)
        p.fields, p.num_fields = arr, len(keep)
        keep = (keep, arr)
    p.file_source_id, p.global_encoding, p.day, p.year = int(file_source_id), int(global_encoding), int(day), int(year)
    for name, value in (("system_identifier", system_identifier), ("generating_software", generating_software)):
        b = os.fsencode(value)
        if len(b) > 32:
            raise ValueError(f"{name}: at most 32 bytes")
        setattr(p, name, b)
    return p, keep


def _las_write_info(info):
    return dict(point_format=int(info.point_format), version_minor=int(info.version_minor), record_length=int(info.record_length),
                header_size=int(info.header_size), scale=tuple(info.scale), offset=tuple(info.offset), min_xyz=tuple(info.min_xyz),
                max_xyz=tuple(info.max_xyz), bounds=tuple(info.bounds), num_records=int(info.num_records),
                by_return=np.array(info.by_return, dtype=np.uint64), out_of_range=int(info.out_of_range),
                clamped_intensity=int(info.clamped_intensity), masked_values=int(info.masked_values), skipped_extras=int(info.skipped_extras))


def _las_write_info_struct(info):
    if isinstance(info, L.LasWriteInfo):
        return info
    s = L.LasWriteInfo()
    s.point_format, s.version_minor = int(info["point_format"]), int(info["version_minor"])
    s.record_length, s.header_size = int(info.get("record_length", 0)), int(info.get("header_size", 0))
    s.num_records = int(info.get("num_records", 0))
    for a in range(3):
        s.scale[a], s.offset[a] = info["scale"][a], info["offset"][a]
        s.min_xyz[a], s.max_xyz[a] = info.get("min_xyz", (0, 0, 0))[a], info.get("max_xyz", (0, 0, 0))[a]
    for k in range(6):
        s.bounds[k] = info.get("bounds", (0.0,) * 6)[k]
    for k in range(15):
        s.by_return[k] = int(info.get("by_return", [0] * 15)[k])
    return s


def _las_extra_arrays(attributes):
    """{name: type string | array} -> (names char**, types int32[], n, keep-alive)."""
    items = list((attributes or {}).items())
    names = [os.fsencode(str(n)) for n, _ in items]
    codes = []
    for _, v in items:
        if isinstance(v, str):
            codes.append(L.ATTR_TYPES[v.lower()][0])
        else:
            a = np.asarray(v)
            match = [t for t, (_, dt, comps) in L.ATTR_TYPES.items() if np.dtype(dt) == a.dtype and comps == (a.shape[1] if a.ndim == 2 else 1)]
            codes.append(L.ATTR_TYPES[match[0]][0] if match else 0)
    types = np.array(codes, dtype=np.int32)
    return (C.c_char_p * max(1, len(names)))(*names), types, len(names), (names, types)


def las_write_check_params(has_intensity=False, attributes=None, **las):
    """What write_las checks of its params against a source with these extras ({name: type string}) before it runs
    (pcv_las_write_check_params_host) -> info dict with the format, version, record length, header size and skipped_extras."""
    pr, _keep = las_write_params(**las)
    names, types, n, _k2 = _las_extra_arrays(attributes)
    info = L.LasWriteInfo()
    _las_check(L.load_library().pcv_las_write_check_params_host(C.byref(pr), int(bool(has_intensity)), names, types.ctypes.data, n, C.byref(info)))
    return _las_write_info(info)


def las_encode_host(points, **las):
    """The host twin of the device packer (pcv_las_encode_host): points as read_las returns them (x, y, z, color or None,
    intensity or None, attributes {name: array}) -> (uint8 array [n, record_length], info dict). **las: las_write_params' keywords."""
    pr, _keep = las_write_params(**las)
    x, y, z = (np.ascontiguousarray(points[k], dtype=np.float64) for k in "xyz")
    n = len(x)
    color = points.get("color")
    color = None if color is None else np.ascontiguousarray(color, dtype=np.uint8)
    inten = points.get("intensity")
    inten = None if inten is None else np.ascontiguousarray(inten, dtype=np.float32)
    attrs = {k: np.ascontiguousarray(v) for k, v in (points.get("attributes") or {}).items()}
    names, types, ne, _k2 = _las_extra_arrays(attrs)
    cols = (C.c_void_p * max(1, ne))(*[a.ctypes.data for a in attrs.values()])
    ptr = lambda a: None if a is None else a.ctypes.data
    lib = L.load_library()
    info = L.LasWriteInfo()
    args = (C.byref(pr), n, ptr(x), ptr(y), ptr(z), ptr(color), ptr(inten), names, types.ctypes.data, cols, ne)
    _las_check(lib.pcv_las_write_check_params_host(C.byref(pr), int(inten is not None), names, types.ctypes.data, ne, C.byref(info)))
    out = np.zeros((n, int(info.record_length)), dtype=np.uint8)
    _las_check(lib.pcv_las_encode_host(*args, out.ctypes.data, out.nbytes, C.byref(info)))
    return out, _las_write_info(info)


def las_write_header(info, **las):
    """The header write_las writes for records that `info` describes (an info dict, or its fields point_format, version_minor,
    scale, offset, num_records, by_return, bounds), as bytes (pcv_las_write_header_host). **las: las_write_params' keywords."""
    pr, _keep = las_write_params(**las)
    s = _las_write_info_struct(info)
    buf, need = C.create_string_buffer(375), C.c_uint64()
    _las_check(L.load_library().pcv_las_write_header_host(C.byref(pr), C.byref(s), buf, 375, C.byref(need)))
    return buf.raw[:need.value]


def las_append_check(path, info, **las):
    """What write_las(open_mode="append") checks before it touches `path` (pcv_las_append_check_host) for a file of `info`'s
    format and version and, unless offset is None, these scale and offset: the file's record count (0: no file)."""
    pr, _keep = las_write_params(**las)
    s = _las_write_info_struct(info)
    old = C.c_uint64()
    _las_check(L.load_library().pcv_las_append_check_host(os.fsencode(str(path)), C.byref(pr), C.byref(s), C.byref(old)))
    return old.value


class LasCloud:
    """A LAS file on the device (Context.las_load): .points is the dict Context.s2_split and build_octree's device path take
    (x, y, z, color[, intensity], attributes) of DeviceColumns; .attributes the extras alone; .info the counts of the load."""

    def __init__(self, ctx, handle):
        self.ctx, self.lib, self.handle = ctx, ctx.lib, handle
        ctx._children.add(self)
        p, info = L.Points(), L.LasInfo()
        self.lib.pcv_las_cloud_points(handle, C.byref(p))
        self.lib.pcv_las_cloud_info(handle, C.byref(info))
        self.info, self.num_points = _las_info(info), int(p.n)
        n = self.num_points
        count, attrs = C.c_uint32(), (L.Attribute * L.LAS_MAX_EXTRAS)()
        self.lib.pcv_las_cloud_attributes(handle, C.byref(count), attrs)
        self.attributes = {}
        for k in range(count.value):
            name = os.fsdecode(attrs[k].name)
            self.attributes[name] = DeviceColumn(self, name, attrs[k].data, n, _LAS_EXTRA_DTYPES[name])
        self.points = dict(x=DeviceColumn(self, "x", p.x, n, np.float64), y=DeviceColumn(self, "y", p.y, n, np.float64),
                           z=DeviceColumn(self, "z", p.z, n, np.float64), color=DeviceColumn(self, "color", p.color, 3 * n, np.uint8))
        if p.intensity:
            self.points["intensity"] = DeviceColumn(self, "intensity", p.intensity, n, np.float32)
        self.points["attributes"] = self.attributes

    def _alive(self):
        if not self.handle:
            raise L.PcvError(L.PCV_E_INVALID, "the LasCloud has been freed")

    def read(self, name):
        """One column as a numpy array (pcv_las_cloud_read): "x", "y", "z", "color" (n, 3), "intensity" or an extra's name."""
        self._alive()
        n = self.num_points
        dtype, count = {"x": ("<f8", n), "y": ("<f8", n), "z": ("<f8", n), "color": ("u1", 3 * n), "intensity": ("<f4", n)}.get(
            name, (_LAS_EXTRA_DTYPES.get(name, "u1"), n))
        a = np.zeros(count, dtype=dtype)
        self.ctx._check(self.lib.pcv_las_cloud_read(self.handle, os.fsencode(name), a.ctypes.data, a.nbytes))
        return a.reshape(-1, 3) if name == "color" else a

    def to_host(self):
        """read_las's dict from the device columns."""
        return dict(x=self.read("x"), y=self.read("y"), z=self.read("z"), color=self.read("color"),
                    intensity=self.read("intensity") if "intensity" in self.points else None,
                    attributes={k: self.read(k) for k in self.attributes}, info=self.info)

    def free(self):
        if getattr(self, "handle", None):
            self.lib.pcv_las_cloud_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def read_ply(path, extras=False):
    """PlyIterator in one pass (src/read_write/ply.rs): dict(x, y, z float64; color (n,3) uint8 or None; intensity or None).
    extras=True (pcv_ply_read_ex): also attributes = {name: array} of every other scalar vertex property in its own type, in the
    form Context.s2_split takes; properties whose name ends in a digit or breaks the naming rules of extras are skipped."""
    lib = L.load_library()
    h = C.c_void_p()
    err = C.create_string_buffer(512)
    rc = lib.pcv_ply_read_ex(str(path).encode(), L.PLY_READ_EXTRAS if extras else 0, C.byref(h), err, 512)
    if rc != L.PCV_OK:
        raise L.PcvError(rc, err.value.decode())
    try:
        p = L.Points()
        lib.pcv_ply_points(h, C.byref(p))
        n = p.n

        def arr(ptr, ctype, count, dtype):
            if not ptr or count == 0:
                return None if not ptr else np.zeros(0, dtype=dtype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(ctype)), shape=(count,)).astype(dtype, copy=True)

        out = dict(x=arr(p.x, C.c_double, n, np.float64), y=arr(p.y, C.c_double, n, np.float64),
                   z=arr(p.z, C.c_double, n, np.float64), color=arr(p.color, C.c_uint8, 3 * n, np.uint8),
                   intensity=arr(p.intensity, C.c_float, n, np.float32))
        if n == 0:
            out["x"] = out["y"] = out["z"] = np.zeros(0)
        if out["color"] is not None:
            out["color"] = out["color"].reshape(-1, 3)
        if extras:
            count, attrs = C.c_uint32(), (L.Attribute * L.S2_MAX_EXTRAS)()
            lib.pcv_ply_attributes(h, C.byref(count), attrs)
            out["attributes"] = {}
            for k in range(count.value):
                dt = np.dtype(L.ATTR_TYPES[L.ATTR_NAMES[attrs[k].data_type]][1])
                col = np.zeros(n, dtype=dt)
                if n:
                    C.memmove(col.ctypes.data, attrs[k].data, n * dt.itemsize)
                out["attributes"][os.fsdecode(attrs[k].name)] = col
        return out
    finally:
        lib.pcv_ply_free(h)


def _is_las(filename):
    try:
        with open(filename, "rb") as f:
            return f.read(4) == b"LASF"
    except OSError:
        return False


def build_octree_from_file(output_directory, resolution, filename, attributes=("color", "intensity"), ctx=None,
                           host_decode=False, **las):
    """Drop-in for reference `build_octree_from_file` (generation.rs:272-287): the vertex records of the file go to the
    device as they are and are decoded there (host_decode=True: the one-pass host parser instead), bounding box on the
    device, build, directory write. Like the reference binary (src/bin/build_octree.rs:47-52) the default attribute
    list asks for intensity; a PLY without it raises (the reference panics)."""
    attributes = tuple(attributes)
    if _is_las(filename):  # LAS: every file has an intensity field; **las are las_params' keywords
        if "color" not in attributes:
            raise ValueError("the octree format requires the 'color' attribute (on_disk.rs:20-22)")
        for a in attributes:
            if a not in ("color", "intensity"):
                raise ValueError(f"unsupported attribute {a!r} (octree/mod.rs:62-74 implies color and intensity)")
        las.setdefault("keep_intensity", "intensity" in attributes)
        ctx = ctx or default_context()
        if host_decode:
            pts = read_las(filename, **las)
            cloud = {k: pts[k] for k in ("x", "y", "z", "color")}
            if pts["intensity"] is not None:
                cloud["intensity"] = pts["intensity"]
            return build_octree(output_directory, resolution, None, cloud, ("color", "intensity") if pts["intensity"] is not None else ("color",), ctx)
        tree = ctx.build_from_las(resolution, filename, **las)
        tree.write_dir(output_directory)
        return tree
    if las:
        raise TypeError(f"{sorted(las)} are keywords for LAS files; {filename!r} is none")
    if not host_decode:
        if "color" not in attributes:
            raise ValueError("the octree format requires the 'color' attribute (on_disk.rs:20-22)")
        for a in attributes:
            if a not in ("color", "intensity"):
                raise ValueError(f"unsupported attribute {a!r} (octree/mod.rs:62-74 implies color and intensity)")
        ctx = ctx or default_context()
        try:
            tree = ctx.build_from_ply(resolution, filename, with_intensity="intensity" in attributes)
        except L.PcvError as e:
            if "requested but the PLY has none" in str(e) or "requires colour" in str(e):
                raise ValueError(str(e)) from None
            raise
        tree.write_dir(output_directory)
        return tree
    pts = read_ply(filename)
    if pts["color"] is None:
        raise ValueError("the PLY has no red/green/blue properties; the octree format requires colour")
    cloud = dict(x=pts["x"], y=pts["y"], z=pts["z"], color=pts["color"])
    if "intensity" in attributes:
        if pts["intensity"] is None:
            raise ValueError("attribute 'intensity' requested but the PLY has none")
        cloud["intensity"] = pts["intensity"]
    return build_octree(output_directory, resolution, None, cloud, attributes, ctx)


_default_ctx = None


class S2QueryBatch(QueryBatch):
    """The result of S2Cloud.query_batch, with QueryBatch's methods: segment k holds the points of cell segments()[1][k] (an
    index into S2Cloud.cells) that location s selected, for the locations (shapes, then unions) one after another. Holds its
    cloud: the cloud's device blobs are read when points are copied out."""
    _prefix = "pcv_s2_query"

    def __init__(self, cloud, handle, num_locations):
        self.tree, self.ctx, self.lib, self.handle = cloud, cloud.ctx, cloud.lib, handle
        self.num_shapes = num_locations
        ns, npt = C.c_uint64(), C.c_uint64()
        self.lib.pcv_s2_query_sizes(handle, C.byref(ns), C.byref(npt))
        self.num_segments, self.num_points = ns.value, npt.value
        self._has_int = cloud.has_intensity
        self._segments = None
        self.ctx._children.add(self)
        cloud._batch_handles[id(self)] = handle

    def free(self):
        # pcv_s2_query_free reads the batch's cloud: a batch that outlives its cloud (both dropped in one garbage collection,
        # finalized in any order; a cloud freed by hand first) was released by S2Cloud.free and must not be freed again
        cloud = self.tree
        if self.handle and self.ctx.handle and cloud.handle:
            self.lib.pcv_s2_query_free(self.handle)
            cloud._batch_handles.pop(id(self), None)
        self.handle = None

    def _ply_available(self):
        have = QueryBatch._ply_available(self)
        have.update(self.tree.attributes)
        return have

    def attribute(self, name, first_segment=0, num_segments=None):
        """One extra attribute of the kept points of segments [first_segment, first_segment + num_segments) (default: to the
        end), in segment order (pcv_s2_query_attribute): a numpy array of the attribute's type, (m,) or (m, 3)."""
        self._live()
        _, _, off = self.segments()
        first = int(first_segment)
        num = self.num_segments - first if num_segments is None else int(num_segments)
        name_b = os.fsencode(name)
        if not (0 <= first <= self.num_segments and 0 <= num <= self.num_segments - first):
            self.ctx._check(self.lib.pcv_s2_query_attribute(self.handle, name_b, max(first, 0), max(num, 0) or (1 << 63), 0, L.MEM_HOST, None))
        m = int(off[first + num] - off[first])
        typ = self.tree.attributes.get(name)
        if typ is None:  # the library's own refusal
            self.ctx._check(self.lib.pcv_s2_query_attribute(self.handle, name_b, first, num, 0, L.MEM_HOST, None))
            raise L.PcvError(L.PCV_E_INVALID, f"Data type for attribute '{name}' not found.")
        _, dtype, comps = L.ATTR_TYPES[typ]
        out = np.zeros((m, comps) if comps > 1 else m, dtype=dtype)
        self.ctx._check(self.lib.pcv_s2_query_attribute(self.handle, name_b, first, num, m, L.MEM_HOST, out.ctypes.data))
        return out


class S2Cloud:
    """An S2 cell cloud held by the library (pcv_s2_cloud): the cells ascending by id and cell-contiguous device blobs."""

    def __init__(self, ctx, handle):
        self.ctx = ctx  # None: opened without a context (s2_open_host), host only
        self.lib = ctx.lib if ctx is not None else L.load_library()
        self.handle = handle
        if ctx is not None:
            ctx._children.add(self)
        nc, n, has_int, level = C.c_uint64(), C.c_uint64(), C.c_int(), C.c_uint32()
        bmin, bmax = (C.c_double * 3)(), (C.c_double * 3)()
        self._check(self.lib.pcv_s2_info(handle, C.byref(nc), C.byref(n), bmin, bmax, C.byref(has_int), C.byref(level)))
        self.num_cells, self.num_points, self.has_intensity, self.split_level = nc.value, n.value, bool(has_int.value), level.value
        self.bbox_min, self.bbox_max = np.array(bmin[:]), np.array(bmax[:])
        self._cells = None
        self._attributes = None
        self._batch_handles = {}  # id(S2QueryBatch) -> its handle, of the batches not yet freed: they go before the cloud does

    def _check(self, rc):
        if self.ctx is not None:
            self.ctx._check(rc)
        else:
            _host_check(rc, "S2Cloud")

    @property
    def attributes(self):
        """The extra attributes: dict name -> type string ("u8" ... "f64", "u8vec3", "f64vec3"), ascending by name
        (pcv_s2_attributes). `color` and `intensity` are the built-in columns and not listed."""
        if self._attributes is None:
            self._alive()
            count = C.c_uint32()
            names, types = (C.c_char_p * L.S2_MAX_EXTRAS)(), (C.c_int32 * L.S2_MAX_EXTRAS)()
            self._check(self.lib.pcv_s2_attributes(self.handle, C.byref(count), names, types))
            self._attributes = {os.fsdecode(names[k]): L.ATTR_NAMES[types[k]] for k in range(count.value)}
        return dict(self._attributes)

    def cell_attribute(self, name, first=0, count=None):
        """One extra attribute of cells [first, first + count) as it stands in their `<token>.<name>` files
        (pcv_s2_cell_attribute): a numpy array of the attribute's type, (m,) or (m, 3)."""
        self._alive()
        count = self.num_cells - first if count is None else count
        if first < 0 or count < 0 or first + count > self.num_cells:
            raise ValueError("cell range past the end")
        name_b = os.fsencode(name)
        typ = self.attributes.get(name)
        if typ is None:  # the library's own refusal
            self._check(self.lib.pcv_s2_cell_attribute(self.handle, name_b, first, count, 0, L.MEM_HOST, None))
            raise L.PcvError(L.PCV_E_INVALID, f"Data type for attribute '{name}' not found.")
        m = int(self.cells[1][first:first + count].sum())
        _, dtype, comps = L.ATTR_TYPES[typ]
        out = np.zeros((m, comps) if comps > 1 else m, dtype=dtype)
        self._check(self.lib.pcv_s2_cell_attribute(self.handle, name_b, first, count, m, L.MEM_HOST, out.ctypes.data))
        return out

    def _alive(self):
        if not self.handle or (self.ctx is not None and not self.ctx.handle):
            raise ValueError("this S2 cell cloud has been freed")

    @property
    def cells(self):
        """(ids, counts, offsets): uint64 arrays, one entry per cell, ascending by id; offsets count points."""
        if self._cells is None:
            self._alive()
            ids, counts, offsets = (np.zeros(self.num_cells, dtype=np.uint64) for _ in range(3))
            self._check(self.lib.pcv_s2_cells(self.handle, ids.ctypes.data, counts.ctypes.data, offsets.ctypes.data))
            self._cells = (ids, counts, offsets)
        return self._cells

    @property
    def order(self):
        """The permutation: order[slot] = input index of the point at `slot` (a stable sort of the input by cell id)."""
        self._alive()
        out = np.zeros(self.num_points, dtype=np.uint32)
        self._check(self.lib.pcv_s2_order(self.handle, out.ctypes.data, L.MEM_HOST))
        return out

    def tokens(self):
        return [s2_cell_token(int(i)) for i in self.cells[0]]

    def cell_points(self, first=0, count=None):
        """(xyz (m, 3) f64, rgb (m, 3) u8, intensity (m,) f32 or None) of cells [first, first + count), as in their files."""
        self._alive()
        count = self.num_cells - first if count is None else count
        if first < 0 or count < 0 or first + count > self.num_cells:
            raise ValueError("cell range past the end")
        m = int(self.cells[1][first:first + count].sum())
        xyz, rgb = np.zeros((m, 3)), np.zeros((m, 3), dtype=np.uint8)
        inten = np.zeros(m, dtype=np.float32) if self.has_intensity else None
        self._check(self.lib.pcv_s2_cell_points(self.handle, first, count, m, L.MEM_HOST, xyz.ctypes.data, rgb.ctypes.data,
                                                    inten.ctypes.data if inten is not None else None))
        return xyz, rgb, inten

    def cells_in_location(self, shapes=None, unions=None):
        """S2Cells::nodes_in_location for every location of one call (pcv_s2_cells_in_location): the prepared `shapes`
        first, then `unions`, each a sequence of cell ids ascending. One uint64 array of cell ids per location, ascending;
        `cells_in_location_indices` gives the same lists as indices into `cells`."""
        return [self.cells[0][idx] for idx in self.cells_in_location_indices(shapes, unions)]

    def cells_in_location_indices(self, shapes=None, unions=None):
        self._alive()
        first, flat = _s2_unions(unions)
        locations = (shapes.count if shapes is not None else 0) + first.size - 1
        capacity = max(1, self.num_cells)
        counts, out = np.zeros(max(1, locations), dtype=np.uint32), np.zeros((max(1, locations), capacity), dtype=np.uint32)
        self._check(self.lib.pcv_s2_cells_in_location(self.handle, shapes.handle if shapes is not None else None, first.size - 1,
                                                          first.ctypes.data, flat.ctypes.data, capacity, counts.ctypes.data, out.ctypes.data))
        return [out[l, :counts[l]].copy() for l in range(locations)]

    def terrain(self, shapes=None, **params):
        """A finished Terrain of the points `shapes` select (None: all points), as OctreeResult.terrain."""
        self._alive()
        return _cloud_terrain(self, shapes, params)

    def map_tiles(self, zoom, min_zoom=None, shapes=None, **params):
        """A finished MapTiles layer of the points `shapes` select (None: all points), as OctreeResult.map_tiles."""
        self._alive()
        return _cloud_map_tiles(self, shapes, zoom, min_zoom, params)

    def query_batch(self, shapes=None, unions=None, intervals=None, filters=None):
        """The points of every location of one call (pcv_s2_query_run): the prepared `shapes`, then `unions`; intervals: None,
        or one entry per location, None or (lo, hi) on intensity. filters (pcv_s2_query_run_ex): None, or one entry per
        location, None or a dict {attribute name: (lo, hi)} of closed intervals on scalar attributes ("intensity" included),
        ANDed; give `intervals` or `filters`, not both. Returns an S2QueryBatch."""
        self._alive()
        first, flat = _s2_unions(unions)
        locations = (shapes.count if shapes is not None else 0) + first.size - 1
        if filters is not None:
            if intervals is not None:
                raise ValueError("query_batch: give intervals or filters, not both (a filter may name 'intensity')")
            filters = list(filters)
            if len(filters) != locations:
                raise ValueError(f"filters: expected {locations} entries (one per location), got {len(filters)}")
            flat_filters = [(l, os.fsencode(name), float(v[0]), float(v[1])) for l, f in enumerate(filters) if f for name, v in f.items()]
            arr = (L.S2Filter * max(1, len(flat_filters)))()
            for k, (l, name_b, lo, hi) in enumerate(flat_filters):
                arr[k].location, arr[k].reserved, arr[k].attribute, arr[k].lo, arr[k].hi = l, 0, name_b, lo, hi
            h = C.c_void_p()
            self._check(self.lib.pcv_s2_query_run_ex(self.handle, shapes.handle if shapes is not None else None, first.size - 1,
                                                     first.ctypes.data, flat.ctypes.data, arr, len(flat_filters), C.byref(h)))
            return S2QueryBatch(self, h, locations)
        iv = used = None
        if intervals is not None:
            intervals = list(intervals)
            if len(intervals) != locations:
                raise ValueError(f"intervals: expected {locations} entries (one per location), got {len(intervals)}")
            iv, used = (C.c_double * max(1, 2 * locations))(), (C.c_uint8 * max(1, locations))()
            for s, v in enumerate(intervals):
                if v is not None:
                    iv[2 * s], iv[2 * s + 1], used[s] = float(v[0]), float(v[1]), 1
        h = C.c_void_p()
        self._check(self.lib.pcv_s2_query_run(self.handle, shapes.handle if shapes is not None else None, first.size - 1, first.ctypes.data,
                                              flat.ctypes.data, iv, used, C.byref(h)))
        return S2QueryBatch(self, h, locations)

    def xray_tiles(self, tile_size_px=256, pixel_size_m=None, strategy="xray", query_from_global=None, intensity_interval=None,
                   background="white", root_node_id="r", max_workspace_bytes=None, min_intensity=0.0, max_intensity=1.0,
                   binning=None, filter_intervals=None):
        """OctreeResult.xray_tiles (same keywords) over this S2 cell cloud (pcv_xray_run_s2_ex): every leaf tile's points are
        those of the cells that cells_in_location lists for the tile's shape, filtered as query_batch filters them.
        binning: None or (name, bin size) on any scalar attribute of the cloud, `intensity` or an extra; filter_intervals:
        None or {name: (lo, hi)}, closed intervals on scalar attributes that every tile's points must lie in.
        Returns an XrayTiles that does not depend on the cloud."""
        if self.ctx is None:
            raise ValueError("xray_tiles: this S2 cell cloud was opened without a context (s2_open_host) and has no device")
        return self.ctx.xray_tiles([self], tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background,
                                   root_node_id, max_workspace_bytes, min_intensity, max_intensity, binning, filter_intervals)

    def xray_quadtree(self, tile_size_px=256, pixel_size_m=None, strategy="xray", query_from_global=None, intensity_interval=None,
                      background="white", root_node_id="r", max_workspace_bytes=None, min_intensity=0.0, max_intensity=1.0,
                      binning=None, output_directory=None, png="stored", filter_intervals=None):
        """xray_tiles (same arguments) with every level above the leaves built on the device, written to output_directory
        when one is given (OctreeResult.xray_quadtree)."""
        xt = self.xray_tiles(tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background, root_node_id,
                             max_workspace_bytes, min_intensity, max_intensity, binning, filter_intervals)
        xt.build_parents()
        if output_directory is not None:
            xt.write(output_directory, png=png)
        return xt

    def write(self, directory):
        """<token>.xyz/.rgb[/.intensity] and <token>.<name> per extra attribute, per cell, + meta.pb (pcv_s2_write_dir)."""
        self._alive()
        self._check(self.lib.pcv_s2_write_dir(self.handle, os.fsencode(directory)))

    def free(self):
        if self.handle and (self.ctx is None or self.ctx.handle):
            for h in self._batch_handles.values():  # plain handles: weak references are gone by the time a collection finalizes
                self.lib.pcv_s2_query_free(h)
            self._batch_handles.clear()
            self.lib.pcv_s2_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class S2Stream:
    """One pcv_s2_stream: `append` is S2Splitter::write for one batch, `finish` its get_meta. A context manager: leaving the
    block on an exception aborts the stream; a stream not finished by the end of the block is aborted too."""

    def __init__(self, ctx, handle):
        self.ctx, self.lib, self.handle = ctx, ctx.lib, handle
        ctx._children.add(self)

    def _alive(self):
        if not self.handle or not self.ctx.handle:
            raise ValueError("this S2 stream is finished")

    def append(self, points):
        """One batch: the SoA dict of s2_split (x=, y=, z=, color=[, intensity=][, attributes=]) or a PointsBatch dict
        (position= (n, 3) f64, color= (n, 3) u8[, intensity= (n,) f32][, attributes=], src/lib.rs:102-107); host arrays or
        device tensors. The first non-empty batch fixes the attribute set (pcv_s2_stream_append_ex)."""
        self._alive()
        if "position" in points:
            pos = points["position"]
            if len(pos.shape) != 2 or pos.shape[1] != 3:
                raise ValueError("position must be (n, 3): one Point3<f64> per row")
            if _is_torch(pos):
                x, y, z = (pos[:, a].contiguous() for a in range(3))
            else:
                pos = np.asarray(pos, dtype=np.float64)
                x, y, z = (np.ascontiguousarray(pos[:, a]) for a in range(3))
        else:
            x, y, z = points["x"], points["y"], points["z"]
        p, keep_alive = self.ctx._points(x, y, z, points["color"], points.get("intensity"))
        attrs, num_attrs, keep_attrs = _attributes(points.get("attributes"), p.n, p.mem == L.MEM_DEVICE)
        self.ctx._check(self.lib.pcv_s2_stream_append_ex(self.handle, C.byref(p), attrs, num_attrs))

    @property
    def info(self):
        """dict(batches, points, cells, pending_points, flushes) so far (pcv_s2_stream_info)."""
        self._alive()
        v = [C.c_uint64() for _ in range(5)]
        self.ctx._check(self.lib.pcv_s2_stream_info(self.handle, *[C.byref(w) for w in v]))
        return dict(zip(("batches", "points", "cells", "pending_points", "flushes"), (w.value for w in v)))

    def _set_memory_cap(self, max_points):
        """For tests (pcv_s2_stream_set_memory_cap): the point limit of an in-memory stream, lowered."""
        self._alive()
        self.ctx._check(self.lib.pcv_s2_stream_set_memory_cap(self.handle, int(max_points)))

    def finish(self):
        """get_meta: the S2Cloud (in directory mode, the directory opened). Consumes the stream, success or not."""
        self._alive()
        h, mine = C.c_void_p(), self.handle
        self.handle = None
        self.ctx._check(self.lib.pcv_s2_stream_finish(mine, C.byref(h)))
        return S2Cloud(self.ctx, h)

    def abort(self):
        if self.handle and self.ctx.handle:
            self.lib.pcv_s2_stream_abort(self.handle)
        self.handle = None

    free = abort  # (Context.close releases its children through free)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        self.abort()
        return False

    def __del__(self):
        try:
            self.abort()
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def s2_merge_plan(parts, chunk_points=0):
    """pcv_s2_merge_plan_host (host only): `parts` = a sequence of (ids, counts), one pair of uint64 arrays per part, ids
    ascending. Returns dict(ids, counts, offsets: the merged cells; segments: a structured array with dst_offset,
    src_offset, part, count, ordered by cell, then part; chunk_first_segment: per output chunk of chunk_points points (0 = the
    kernel's) the segment that holds its first point)."""
    parts = [(np.ascontiguousarray(i, dtype=np.uint64).ravel(), np.ascontiguousarray(c, dtype=np.uint64).ravel()) for i, c in parts]
    for i, c in parts:
        if i.size != c.size:
            raise ValueError("a part's ids and counts must have the same length")
    first = np.zeros(len(parts) + 1, dtype=np.uint64)
    first[1:] = np.cumsum([i.size for i, _ in parts], dtype=np.uint64)
    ids = np.concatenate([i for i, _ in parts]) if parts else np.zeros(0, dtype=np.uint64)
    counts = np.concatenate([c for _, c in parts]) if parts else np.zeros(0, dtype=np.uint64)
    lib = L.load_library()
    nc, ns, nk = C.c_uint64(), C.c_uint64(), C.c_uint64()

    def call(*arrays):
        _host_check(lib.pcv_s2_merge_plan_host(len(parts), first.ctypes.data, ids.ctypes.data, counts.ctypes.data, int(chunk_points),
                                               C.byref(nc), C.byref(ns), C.byref(nk), *arrays), "pcv_s2_merge_plan_host")
    call(None, None, None, None, None)
    out_ids, out_counts, out_offsets = (np.zeros(nc.value, dtype=np.uint64) for _ in range(3))
    segments = np.zeros(ns.value, dtype=np.dtype([("dst_offset", "<u8"), ("src_offset", "<u8"), ("part", "<u4"), ("count", "<u4")]))
    chunk_first = np.zeros(nk.value, dtype=np.uint64)
    call(out_ids.ctypes.data, out_counts.ctypes.data, out_offsets.ctypes.data, segments.ctypes.data, chunk_first.ctypes.data)
    return dict(ids=out_ids, counts=out_counts, offsets=out_offsets, segments=segments, chunk_first_segment=chunk_first)


def _host_check(rc, what):
    if rc != L.PCV_OK:
        msg = L.load_library().pcv_host_last_error()
        raise L.PcvError(rc, (msg.decode() if msg else "") or what)


def s2_cell_ids(x, y, z, level=30):
    """pcv_s2_cell_ids_host (host only): CellID::from_point(p).parent(level) per point, the chain the device runs."""
    x, y, z = _wmr_xyz(x, y, z)
    ids = np.zeros(x.size, dtype=np.uint64)
    if not 0 <= int(level) <= 0xFFFFFFFF:
        raise L.PcvError(L.PCV_E_INVALID, "an S2 level is 0 ..= 30")
    _host_check(L.load_library().pcv_s2_cell_ids_host(x.size, x.ctypes.data, y.ctypes.data, z.ctypes.data, int(level), ids.ctypes.data),
                "pcv_s2_cell_ids_host")
    return ids


def s2_cell_token(cell_id):
    """CellID::to_token: the stem of a cell's files."""
    out = C.create_string_buffer(17)
    _host_check(L.load_library().pcv_s2_cell_token(int(cell_id), out), "pcv_s2_cell_token")
    return out.value.decode()


def s2_union_contains(cells, x, y, z):
    """pcv_s2_union_contains_host (host only): CellUnion::contains per point for cell ids ascending, as uint8 flags."""
    cells = np.ascontiguousarray(cells, dtype=np.uint64).ravel()
    x, y, z = _wmr_xyz(x, y, z)
    keep = np.zeros(x.size, dtype=np.uint8)
    _host_check(L.load_library().pcv_s2_union_contains_host(cells.ctypes.data, cells.size, x.size, x.ctypes.data, y.ctypes.data,
                                                            z.ctypes.data, keep.ctypes.data), "pcv_s2_union_contains_host")
    return keep


def s2_check_attributes(attributes):
    """pcv_s2_attributes_check_host (host only): the rules of s2_split's `attributes` on a dict name -> type string (or a
    proto enum value); raises PcvError (PCV_E_INVALID) naming the attribute that breaks one."""
    arr, keep = (L.Attribute * max(1, len(attributes)))(), []
    for k, (name, typ) in enumerate(attributes.items()):
        name_b = name if isinstance(name, bytes) else os.fsencode(name)
        keep.append(name_b)
        arr[k].name, arr[k].data_type = name_b, typ if isinstance(typ, int) else L.ATTR_TYPES.get(str(typ).lower(), (0,))[0]
    _host_check(L.load_library().pcv_s2_attributes_check_host(arr, len(attributes)), "pcv_s2_attributes_check_host")


def s2_filter_keep(dtype, data, lo, hi, keep=None):
    """pcv_s2_filter_keep_host (host only): the filter test of S2Cloud.query_batch for one scalar attribute — `data` as f64
    (Rust's `as f64`) in [lo, hi] — ANDed into `keep` (uint8, default all ones), which is returned. dtype: a type string of
    S2Cloud.attributes; a vector type is refused."""
    typ = str(dtype).lower()
    if typ not in L.ATTR_TYPES:
        raise L.PcvError(L.PCV_E_INVALID, "Attribute data type invalid")
    code, np_dtype, comps = L.ATTR_TYPES[typ]
    data = np.asarray(data)
    if comps == 1:
        if data.dtype.itemsize != np.dtype(np_dtype).itemsize:
            raise TypeError(f"s2_filter_keep: dtype {data.dtype} is not of type {typ}")
        data = np.ascontiguousarray(data).ravel()
    n = data.shape[0]
    keep = np.ones(n, dtype=np.uint8) if keep is None else np.ascontiguousarray(keep, dtype=np.uint8)
    if keep.size != n:
        raise ValueError("keep must hold one byte per value")
    data = np.ascontiguousarray(data)
    _host_check(L.load_library().pcv_s2_filter_keep_host(code, n, data.ctypes.data, float(lo), float(hi), keep.ctypes.data), "pcv_s2_filter_keep_host")
    return keep


def _s2_unions(unions):
    """(union_first uint32[U + 1], union_cells uint64) of a sequence of cell-id sequences."""
    unions = [np.ascontiguousarray(u, dtype=np.uint64).ravel() for u in (unions if unions is not None else [])]
    first = np.zeros(len(unions) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([u.size for u in unions], dtype=np.uint64)
    flat = np.ascontiguousarray(np.concatenate(unions) if unions else np.zeros(0), dtype=np.uint64)
    return first, flat


def _polygon_rings(rings):
    """(ring_first uint32[R + 1], vertices float64 (V, 2)) of one (k, 2) array or a sequence of them."""
    if isinstance(rings, np.ndarray) and rings.ndim == 2:
        rings = [rings]
    rings = [np.ascontiguousarray(r, dtype=np.float64).reshape(-1, 2) for r in rings]
    first = np.zeros(len(rings) + 1, dtype=np.uint32)
    first[1:] = np.cumsum([r.shape[0] for r in rings], dtype=np.uint64)
    verts = np.ascontiguousarray(np.concatenate(rings) if rings else np.zeros((0, 2)), dtype=np.float64)
    return first, verts


def _polygon_table(polygons):
    """(polygon_first, ring_first, vertices) of a sequence of polygons, as pcv_shapes_create_ex2 takes them."""
    parts = [_polygon_rings(p) for p in polygons]
    pfirst = np.zeros(len(parts) + 1, dtype=np.uint32)
    pfirst[1:] = np.cumsum([f.size - 1 for f, _ in parts], dtype=np.uint64)
    rfirst, at = [np.zeros(1, dtype=np.uint32)], 0
    for f, v in parts:
        rfirst.append((f[1:].astype(np.uint64) + at).astype(np.uint32))
        at += v.shape[0]
    verts = np.ascontiguousarray(np.concatenate([v for _, v in parts]) if parts else np.zeros((0, 2)), dtype=np.float64)
    return pfirst, np.ascontiguousarray(np.concatenate(rfirst), dtype=np.uint32), verts


def polygon_check(rings, frame=0, z_min=-np.inf, z_max=np.inf):
    """pcv_polygon_check_host: what Context.shapes checks of a polygon; raises PcvError with the message."""
    first, verts = _polygon_rings(rings)
    _host_check(L.load_library().pcv_polygon_check_host(first.size - 1, first.ctypes.data, verts.ctypes.data, int(frame), float(z_min),
                                                        float(z_max)), "pcv_polygon_check_host")


def polygon_contains(rings, x, y, z, frame=0, z_min=-np.inf, z_max=np.inf):
    """pcv_polygon_contains_host: the keep flag of every point, as uint8 — frame 0: the point rule on (x, y) and the closed
    height range on z; frame 1: the rule on the web-mercator projection of the ECEF point. Bit for bit the device's."""
    first, verts = _polygon_rings(rings)
    x, y, z = _wmr_xyz(x, y, z)
    keep = np.zeros(x.size, dtype=np.uint8)
    _host_check(L.load_library().pcv_polygon_contains_host(first.size - 1, first.ctypes.data, verts.ctypes.data, int(frame), float(z_min),
                                                           float(z_max), x.size, x.ctypes.data, y.ctypes.data, z.ctypes.data,
                                                           keep.ctypes.data), "pcv_polygon_contains_host")
    return keep


def polygon_intersects_cubes(rings, cubes, z_min=-np.inf, z_max=np.inf):
    """pcv_polygon_intersects_cubes_host: the node rule of an xy-frame polygon per cube (n x 4: min xyz, edge), as uint8 flags —
    the predicate its node list over an octree is the breadth-first walk of."""
    first, verts = _polygon_rings(rings)
    cubes = np.ascontiguousarray(cubes, dtype=np.float64).reshape(-1, 4)
    out = np.zeros(cubes.shape[0], dtype=np.uint8)
    _host_check(L.load_library().pcv_polygon_intersects_cubes_host(first.size - 1, first.ctypes.data, verts.ctypes.data, float(z_min),
                                                                   float(z_max), cubes.shape[0], cubes.ctypes.data, out.ctypes.data),
                "pcv_polygon_intersects_cubes_host")
    return out


def polygon_from_lat_lng(rings_deg):
    """Rings of (latitude, longitude) in degrees as rings of normalized web-mercator (x, y), for ("polygon_web_mercator", rings):
    wmr_from_lat_lng per vertex."""
    if isinstance(rings_deg, np.ndarray) and rings_deg.ndim == 2:
        rings_deg = [rings_deg]
    out = []
    for r in rings_deg:
        r = np.asarray(r, dtype=np.float64).reshape(-1, 2)
        u, v = wmr_from_lat_lng(np.radians(r[:, 0]), np.radians(r[:, 1]))
        out.append(np.stack([u, v], axis=1))
    return out


def s2_cell_geometry(cell_id):
    """pcv_s2_cell_geometry_host: dict(rect (4), center (lat, lng), uv (4), vertices (4, 3), vertex_lat_lng (4, 2)) of a cell of
    level 1 ..= 30, as Rect::intersects_cell reads it."""
    g = np.zeros(30)
    _host_check(L.load_library().pcv_s2_cell_geometry_host(int(cell_id), g.ctypes.data), "pcv_s2_cell_geometry_host")
    return dict(rect=g[0:4], center=g[4:6], uv=g[6:10], vertices=g[10:22].reshape(4, 3), vertex_lat_lng=g[22:30].reshape(4, 2))


def s2_cell_rect(cell_id):
    """pcv_s2_cell_rect_host: Cell::rect_bound as (lat.lo, lat.hi, lng.lo, lng.hi)."""
    r = np.zeros(4)
    _host_check(L.load_library().pcv_s2_cell_rect_host(int(cell_id), r.ctypes.data), "pcv_s2_cell_rect_host")
    return r


def s2_corners_rect(corners):
    """pcv_s2_corners_rect_host: the rect of cells_in_convex_polyhedron for the (8, 3) corners of a shape."""
    c = np.ascontiguousarray(corners, dtype=np.float64).ravel()
    if c.size != 24:
        raise ValueError("corners must be (8, 3)")
    r = np.zeros(4)
    _host_check(L.load_library().pcv_s2_corners_rect_host(c.ctypes.data, r.ctypes.data), "pcv_s2_corners_rect_host")
    return r


def s2_rect_intersects_cell(rect, cell_id):
    """pcv_s2_rect_intersects_cell_host: Rect::intersects_cell."""
    r = np.ascontiguousarray(rect, dtype=np.float64).ravel()
    if r.size != 4:
        raise ValueError("a rect is (lat.lo, lat.hi, lng.lo, lng.hi)")
    out = C.c_int()
    _host_check(L.load_library().pcv_s2_rect_intersects_cell_host(r.ctypes.data, int(cell_id), C.byref(out)), "pcv_s2_rect_intersects_cell_host")
    return bool(out.value)


def s2_union_normalize(cells):
    """pcv_s2_union_normalize_host: CellUnion::normalize of cell ids in any order, as a new uint64 array."""
    c = np.array(cells, dtype=np.uint64).ravel()
    n = C.c_uint32(c.size)
    _host_check(L.load_library().pcv_s2_union_normalize_host(c.ctypes.data, C.byref(n)), "pcv_s2_union_normalize_host")
    return c[:n.value].copy()


def s2_union_intersects(cells, ids):
    """pcv_s2_union_intersects_host: CellUnion::intersects_cellid per id for cell ids ascending, as uint8 flags."""
    cells = np.ascontiguousarray(cells, dtype=np.uint64).ravel()
    ids = np.ascontiguousarray(ids, dtype=np.uint64).ravel()
    out = np.zeros(ids.size, dtype=np.uint8)
    _host_check(L.load_library().pcv_s2_union_intersects_host(cells.ctypes.data, cells.size, ids.size, ids.ctypes.data, out.ctypes.data),
                "pcv_s2_union_intersects_host")
    return out


def s2_union_intersects_cubes(cells, cubes):
    """pcv_s2_union_intersects_cubes_host: cells_intersecting_polyhedron(cells, cube) per cube (n x 4: min xyz, edge) for cell
    ids ascending, of level 1 or finer, as uint8 flags — the predicate a cell union's node list over an octree is the
    breadth-first walk of."""
    cells = np.ascontiguousarray(cells, dtype=np.uint64).ravel()
    cubes = np.ascontiguousarray(cubes, dtype=np.float64).reshape(-1, 4)
    out = np.zeros(cubes.shape[0], dtype=np.uint8)
    _host_check(L.load_library().pcv_s2_union_intersects_cubes_host(cells.ctypes.data, cells.size, cubes.shape[0], cubes.ctypes.data,
                                                                    out.ctypes.data), "pcv_s2_union_intersects_cubes_host")
    return out


def s2_cells_in_location(cell_ids, kinds=None, valid=None, corners=None, unions=None):
    """pcv_s2_cells_in_location_host: the lists of S2Cloud.cells_in_location_indices over plain arrays — the cloud's cell ids
    (ascending); per shape its PCV_SHAPE_* kind, valid flag and (8, 3) corners (Shapes.kinds, Shapes.get); then the unions."""
    ids = np.ascontiguousarray(cell_ids, dtype=np.uint64).ravel()
    kinds = np.ascontiguousarray(kinds if kinds is not None else [], dtype=np.int32).ravel()
    valid = np.ascontiguousarray(valid if valid is not None else np.ones(kinds.size), dtype=np.int32).ravel()
    corners = np.ascontiguousarray(corners if corners is not None else np.zeros((0, 8, 3)), dtype=np.float64).reshape(-1, 24)
    if not (kinds.size == valid.size == corners.shape[0]):
        raise ValueError("kinds, valid and corners differ in length")
    first, flat = _s2_unions(unions)
    locations = kinds.size + first.size - 1
    capacity = max(1, ids.size)
    counts, out = np.zeros(max(1, locations), dtype=np.uint32), np.zeros((max(1, locations), capacity), dtype=np.uint32)
    _host_check(L.load_library().pcv_s2_cells_in_location_host(ids.size, ids.ctypes.data, kinds.size, kinds.ctypes.data, valid.ctypes.data,
                                                               corners.ctypes.data, first.size - 1, first.ctypes.data, flat.ctypes.data,
                                                               capacity, counts.ctypes.data, out.ctypes.data), "pcv_s2_cells_in_location_host")
    return [out[l, :counts[l]].copy() for l in range(locations)]


def s2_open_host(directory):
    """pcv_s2_open_dir without a context (no device): an S2Cloud that serves cells, cell_points and write only."""
    h = C.c_void_p()
    _host_check(L.load_library().pcv_s2_open_dir(None, os.fsencode(str(directory)), C.byref(h)), "pcv_s2_open_dir")
    return S2Cloud(None, h)


# ---- terrain layers (pcv_terrain_*) ----
def terrain_params(tile_size=256, resolution_m=None, origin=(0.0, 0.0, 0.0), world_from_terrain=None, statistic="max", min_points=1,
                   max_pool_bytes=None, staging_points=0):
    """pcv_terrain_params. world_from_terrain: None (identity) or translation xyz + unit quaternion ijkw; statistic: "max" |
    "min" | "mean" (or the number); max_pool_bytes None: the default of 2 GiB. Nothing is checked here: the library does."""
    if resolution_m is None:
        raise ValueError("resolution_m is required")
    pr = L.TerrainParams()
    pr.tile_size = int(tile_size)
    pr.statistic = L.TERRAIN_STATISTICS[statistic] if isinstance(statistic, str) else int(statistic)
    pr.resolution_m = float(resolution_m)
    iso = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0] if world_from_terrain is None else [float(v) for v in world_from_terrain]
    if len(iso) != 7 or len(origin) != 3:
        raise ValueError("world_from_terrain: translation xyz + quaternion ijkw (7 numbers); origin: 3 numbers")
    for a in range(3):
        pr.origin[a] = float(origin[a])
    for a in range(7):
        pr.world_from_terrain[a] = iso[a]
    pr.min_points, pr.reserved = int(min_points), 0
    pr.max_pool_bytes = 0 if max_pool_bytes is None else int(max_pool_bytes)
    pr.staging_points = int(staging_points)
    return pr


def _terrain_pr(params):
    return params if isinstance(params, L.TerrainParams) else terrain_params(**params)


def terrain_check_params(params):
    """pcv_terrain_check_params_host: raises PcvError with the rule that is broken."""
    _host_check(L.load_library().pcv_terrain_check_params_host(C.byref(_terrain_pr(params))), "pcv_terrain_check_params_host")


def terrain_frame(params):
    """terrain_from_world as (M [3, 3], t [3]): l = M (p - t) (pcv_terrain_frame_host)."""
    out = np.zeros(12)
    _host_check(L.load_library().pcv_terrain_frame_host(C.byref(_terrain_pr(params)), out.ctypes.data), "pcv_terrain_frame_host")
    return out[:9].reshape(3, 3).copy(), out[9:].copy()


def terrain_vertex(params, x, y, z):
    """The grid chain on the host (pcv_terrain_vertex_host), the kernels' twin: (i, j as int64, h as float32, ok as bool)."""
    x, y, z = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (x, y, z))
    n = x.size
    if y.size != n or z.size != n:
        raise ValueError("x, y, z must have the same length")
    i, j = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    h, ok = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.uint8)
    _host_check(L.load_library().pcv_terrain_vertex_host(C.byref(_terrain_pr(params)), n, x.ctypes.data, y.ctypes.data, z.ctypes.data,
                                                         i.ctypes.data, j.ctypes.data, h.ctypes.data, ok.ctypes.data), "pcv_terrain_vertex_host")
    return i, j, h, ok.astype(bool)


def terrain_quad_masks(is_set, i0=0, j0=0):
    """The quad masks (uint32 [h, w]) of a window of set flags [h, w] (row = j - j0, column = i - i0) whose first vertex is
    (i0, j0); nothing outside the window is set (pcv_terrain_quad_masks_host)."""
    flags = np.ascontiguousarray(np.asarray(is_set) != 0, dtype=np.uint8)
    if flags.ndim != 2:
        raise ValueError("is_set: a 2-D array")
    out = np.zeros(flags.shape, dtype=np.uint32)
    _host_check(L.load_library().pcv_terrain_quad_masks_host(int(i0), int(j0), flags.shape[1], flags.shape[0], flags.ctypes.data,
                                                             out.ctypes.data), "pcv_terrain_quad_masks_host")
    return out


def terrain_tile_name(x, y):
    """'x{:08}_y{:08}' of a tile position, the sign counting toward the width (pcv_terrain_tile_name_host)."""
    buf = C.create_string_buffer(32)
    _host_check(L.load_library().pcv_terrain_tile_name_host(int(x), int(y), buf, 32), "pcv_terrain_tile_name_host")
    return buf.value.decode()


def terrain_meta_json(params, tile_positions=()):
    """The text of meta.json (pcv_terrain_meta_json_host)."""
    pos = np.ascontiguousarray(np.asarray(tile_positions, dtype=np.int32).reshape(-1, 2))
    lib, pr, n = L.load_library(), _terrain_pr(params), C.c_uint64()
    _host_check(lib.pcv_terrain_meta_json_host(C.byref(pr), pos.shape[0], pos.ctypes.data, None, 0, C.byref(n)), "pcv_terrain_meta_json_host")
    buf = C.create_string_buffer(n.value + 1)
    _host_check(lib.pcv_terrain_meta_json_host(C.byref(pr), pos.shape[0], pos.ctypes.data, buf, n.value, C.byref(n)), "pcv_terrain_meta_json_host")
    return buf.raw[:n.value].decode()


def read_terrain(directory):
    """A terrain directory as the viewer's reader takes it (terrain_drawer/read_write.rs), in pure Python: dict(tile_size,
    world_from_terrain [7: translation xyz, quaternion ijkw], origin, resolution_m, tiles int32 [n, 2], heights float32
    [n, T, T, 2] (height, quad mask), colors uint8 [n, T, T, 4])."""
    import json
    with open(os.path.join(str(directory), "meta.json")) as f:
        meta = json.load(f)
    T = int(meta["tile_size"])
    tiles = np.asarray(meta["tile_positions"], dtype=np.int32).reshape(-1, 2)
    heights = np.zeros((tiles.shape[0], T, T, 2), dtype=np.float32)
    colors = np.zeros((tiles.shape[0], T, T, 4), dtype=np.uint8)
    for k, (x, y) in enumerate(tiles):
        name = os.path.join(str(directory), f"x{int(x):08d}_y{int(y):08d}")
        h = np.fromfile(name + ".height", dtype="<f4")
        c = np.fromfile(name + ".color", dtype=np.uint8)
        if h.size != T * T * 2 or c.size != T * T * 4:
            raise L.PcvError(L.PCV_E_IO, f"{name}: a tile of {T} x {T} vertices has {T * T * 8} height and {T * T * 4} colour bytes")
        heights[k], colors[k] = h.reshape(T, T, 2), c.reshape(T, T, 4)
    iso = meta["world_from_terrain"]
    return dict(tile_size=T, world_from_terrain=np.array(list(iso["translation"]) + list(iso["rotation"]), dtype=np.float64),
                origin=np.array(meta["origin"], dtype=np.float64), resolution_m=float(meta["resolution_m"]), tiles=tiles,
                heights=heights, colors=colors)


class Terrain:
    """One pcv_terrain: points in (add_points / add), finish, then the tiles with a set vertex — ascending by (x, y) — as
    arrays or as the directory sdl_viewer --terrain reads."""

    def __init__(self, ctx, handle, params):
        self.ctx, self.lib, self.handle, self.params = ctx, ctx.lib, handle, params
        self.tile_size = int(params.tile_size)
        ctx._children.add(self)

    def _live(self):
        if not self.handle or not self.ctx.handle:
            raise L.PcvError(L.PCV_E_INVALID, "the terrain was freed")

    def add_points(self, x, y, z, rgb):
        """f64 planes and 3-byte colours, numpy arrays or torch device tensors (pcv_terrain_add_points)."""
        self._live()
        bufs = [_Buf(x, np.float64, "x"), _Buf(y, np.float64, "y"), _Buf(z, np.float64, "z"), _Buf(rgb, np.uint8, "rgb")]
        n = bufs[0].size
        if bufs[1].size != n or bufs[2].size != n or bufs[3].size != 3 * n:
            raise ValueError("x, y, z of n points and rgb of 3 n bytes")
        if len({b.device for b in bufs}) != 1:
            raise ValueError("all point arrays must live in the same memory space")
        if bufs[0].device:
            self.ctx.wait_torch()
        self.ctx._check(self.lib.pcv_terrain_add_points(self.handle, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                                        L.MEM_DEVICE if bufs[0].device else L.MEM_HOST))
        return self

    def add(self, batch, shape=None, first_segment=0, num_segments=None):
        """The points of a QueryBatch or S2QueryBatch: of shape `shape`, or of a segment range (default: all), pulled through
        a bounded staging buffer on the device (pcv_terrain_add_query_batch / pcv_terrain_add_s2_query)."""
        self._live()
        batch._live()
        first, num = batch._ply_range(shape, first_segment, num_segments)
        fn = self.lib.pcv_terrain_add_s2_query if isinstance(batch, S2QueryBatch) else self.lib.pcv_terrain_add_query_batch
        self.ctx._check(fn(self.handle, batch.handle, first, num))
        return self

    def finish(self):
        self._live()
        self.ctx._check(self.lib.pcv_terrain_finish(self.handle))
        return self

    def info(self):
        self._live()
        inf = L.TerrainInfo()
        self.ctx._check(self.lib.pcv_terrain_info_get(self.handle, C.byref(inf)))
        return dict(points_added=inf.points_added, outside=inf.outside, set_vertices=inf.set_vertices, rendered_quads=inf.rendered_quads,
                    tiles=inf.tiles, pool_bytes=inf.pool_bytes, vertex_min=tuple(inf.vertex_min), vertex_max=tuple(inf.vertex_max),
                    finished=bool(inf.finished))

    def tiles(self):
        """Tile positions, int32 [n, 2], ascending by (x, y)."""
        self._live()
        n = C.c_uint64()
        self.ctx._check(self.lib.pcv_terrain_tiles(self.handle, 0, None, C.byref(n)))
        out = np.zeros((n.value, 2), dtype=np.int32)
        self.ctx._check(self.lib.pcv_terrain_tiles(self.handle, n.value, out.ctypes.data, C.byref(n)))
        return out

    def _plane(self, fn, first_tile, num_tiles, tail, dtype, device):
        self._live()
        n = C.c_uint64()
        self.ctx._check(self.lib.pcv_terrain_tiles(self.handle, 0, None, C.byref(n)))
        first = int(first_tile)
        num = max(n.value - first, 0) if num_tiles is None else int(num_tiles)
        T = self.tile_size
        if not (0 <= first <= n.value and 0 <= num <= n.value - first):
            raise L.PcvError(L.PCV_E_INVALID, f"tile range past the end: tiles [{first}, {first + num}) of {n.value}")
        if device:
            import torch
            out = torch.empty((num, T, T) + tail, dtype=getattr(torch, np.dtype(dtype).name), device=f"cuda:{self.ctx.device}")
            self.ctx.wait_torch()
            ptr, mem = out.data_ptr(), L.MEM_DEVICE
        else:
            out = np.zeros((num, T, T) + tail, dtype=dtype)
            ptr, mem = out.ctypes.data, L.MEM_HOST
        if num:
            self.ctx._check(fn(self.handle, first, num, mem, ptr))
        return out

    def heights(self, first_tile=0, num_tiles=None, device=False):
        """float32 [n, T, T, 2]: height and quad mask; row = j mod T, column = i mod T."""
        return self._plane(self.lib.pcv_terrain_heights, first_tile, num_tiles, (2,), np.float32, device)

    def colors(self, first_tile=0, num_tiles=None, device=False):
        """uint8 [n, T, T, 4]: r g b 255 of a set vertex, zeros of an unset one."""
        return self._plane(self.lib.pcv_terrain_colors, first_tile, num_tiles, (4,), np.uint8, device)

    def counts(self, first_tile=0, num_tiles=None, device=False):
        """[n, T, T] points per vertex (uint32; int32 bits on the device, torch having no uint32 everywhere)."""
        return self._plane(self.lib.pcv_terrain_counts, first_tile, num_tiles, (), np.int32 if device else np.uint32, device)

    def write(self, directory):
        """The directory sdl_viewer --terrain reads: meta.json and x{:08}_y{:08}.height / .color per tile."""
        self._live()
        self.ctx._check(self.lib.pcv_terrain_write_dir(self.handle, os.fsencode(str(directory))))

    def free(self):
        if self.handle and self.ctx.handle:
            self.lib.pcv_terrain_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _cloud_bbox(cloud):
    if isinstance(cloud, S2Cloud):
        return cloud.bbox_min, cloud.bbox_max
    m = cloud.meta()
    return m["bbox_min"], m["bbox_max"]


def _cloud_terrain(cloud, shapes, params, into=None):
    """The points `shapes` select from an octree or an S2 cloud (None: all) into `into`, or into a new finished Terrain."""
    ctx = cloud.ctx
    own = shapes is None
    if own:
        shapes = ctx.shapes([("all",)])
    batch = t = None
    try:
        batch = cloud.query_batch(shapes)
        t = into if into is not None else ctx.terrain_begin(*_cloud_bbox(cloud), **params)
        t.add(batch)
        return t if into is not None else t.finish()
    except Exception:
        if t is not None and into is None:
            t.free()
        raise
    finally:
        if batch is not None:
            batch.free()
        if own:
            shapes.free()


def build_terrain(ctx, point_cloud_locations, output_directory, **params):
    """A terrain directory from cloud directories: the kind of the first one (cloud_kind) decides, every directory is opened
    as that kind, all their points go into one grid over the union of their boxes, and the layer is written to
    output_directory. params: terrain_params' arguments. Returns the finished Terrain."""
    locations = list(point_cloud_locations)
    if not locations:
        raise ValueError("No locations specified for point cloud client.")
    opener = ctx.s2_open if cloud_kind(locations[0]) == "s2" else ctx.open_dir
    clouds = [opener(d) for d in locations]
    t = None
    try:
        boxes = [_cloud_bbox(c) for c in clouds]
        lo, hi = np.min([b[0] for b in boxes], axis=0), np.max([b[1] for b in boxes], axis=0)
        t = ctx.terrain_begin(lo, hi, **params)
        for c in clouds:
            _cloud_terrain(c, None, params, into=t)
        t.finish()
        t.write(output_directory)
        return t
    except Exception:
        if t is not None:
            t.free()
        raise
    finally:
        for c in clouds:
            c.free()


# ---- map tiles (pcv_maptiles_*) ----
def map_tiles_params(zoom, background=(0, 0, 0, 0), max_tiles=1 << 20, max_pool_bytes=0, staging_points=0):
    """pcv_maptiles_params. background: (r, g, b, a) or the packed RGBA8 integer, transparent black by default."""
    pr = L.MapTilesParams()
    pr.zoom = int(zoom)
    if isinstance(background, (int, np.integer)):
        pr.background = int(background)
    else:
        r, g, b, a = (int(v) & 255 for v in background)
        pr.background = r | g << 8 | b << 16 | a << 24
    pr.max_tiles, pr.max_pool_bytes, pr.staging_points = int(max_tiles), int(max_pool_bytes), int(staging_points)
    return pr


def map_tiles_check_params(zoom, min_zoom=None, **params):
    """pcv_maptiles_check_params_host: raises PcvError with the rule that is broken."""
    pr = map_tiles_params(zoom, **params)
    _host_check(L.load_library().pcv_maptiles_check_params_host(C.byref(pr), int(zoom if min_zoom is None else min_zoom)),
                "pcv_maptiles_check_params_host")


def map_tile_pixels(zoom, x, y, z):
    """The pixel rule on the host (pcv_maptiles_pixels_host), the kernels' twin: (gx, gy as uint32 global pixels at `zoom`,
    ok as bool: False where the point is dropped). The tile is (gx >> 8, gy >> 8), the pixel in it (gx & 255, gy & 255)."""
    x, y, z = (np.ascontiguousarray(v, dtype=np.float64).ravel() for v in (x, y, z))
    n = x.size
    if y.size != n or z.size != n:
        raise ValueError("x, y, z of n points")
    gx, gy, ok = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    _host_check(L.load_library().pcv_maptiles_pixels_host(int(zoom), n, x.ctypes.data, y.ctypes.data, z.ctypes.data, gx.ctypes.data,
                                                          gy.ctypes.data, ok.ctypes.data), "pcv_maptiles_pixels_host")
    return gx, gy, ok.astype(bool)


def map_tile_quad_index(zoom, x, y):
    """The xray quadtree index of slippy tile (x, y) at `zoom` (pcv_maptiles_quad_index_host)."""
    out = C.c_uint64()
    _host_check(L.load_library().pcv_maptiles_quad_index_host(int(zoom), int(x), int(y), C.byref(out)), "pcv_maptiles_quad_index_host")
    return out.value


def map_tile_from_quad_index(zoom, index):
    """The slippy tile (x, y) of an xray quadtree index at `zoom` (pcv_maptiles_quad_tile_host)."""
    x, y = C.c_uint32(), C.c_uint32()
    _host_check(L.load_library().pcv_maptiles_quad_tile_host(int(zoom), int(index), C.byref(x), C.byref(y)), "pcv_maptiles_quad_tile_host")
    return x.value, y.value


def map_tiles_json(tiles):
    """The text of tiles.json (pcv_maptiles_json_host) for {zoom: [[x, y], ...]} over a contiguous range of zooms."""
    zooms = sorted(int(z) for z in tiles)
    if not zooms or zooms != list(range(zooms[0], zooms[-1] + 1)):
        raise ValueError("tiles: a dict over a contiguous, non-empty range of zooms")
    lists = [np.asarray(tiles[z], dtype=np.uint32).reshape(-1, 2) for z in zooms]
    counts = np.array([len(t) for t in lists], dtype=np.uint64)
    xy = np.ascontiguousarray(np.concatenate(lists, axis=0))
    lib, n = L.load_library(), C.c_uint64()
    _host_check(lib.pcv_maptiles_json_host(zooms[0], zooms[-1], counts.ctypes.data, xy.ctypes.data, None, 0, C.byref(n)), "pcv_maptiles_json_host")
    buf = C.create_string_buffer(n.value + 1)
    _host_check(lib.pcv_maptiles_json_host(zooms[0], zooms[-1], counts.ctypes.data, xy.ctypes.data, buf, n.value, C.byref(n)), "pcv_maptiles_json_host")
    return buf.raw[:n.value].decode()


def read_map_tiles(directory):
    """A map-tile directory in pure Python plus the library's PNG reader: dict(scheme, format, tile_size, minzoom, maxzoom,
    bounds [west, south, east, north] in degrees, tiles {zoom: uint32 [n, 2]}, images {zoom: uint8 [n, 256, 256, 4]})."""
    import json
    directory = str(directory)
    with open(os.path.join(directory, "tiles.json")) as f:
        meta = json.load(f)
    T = int(meta["tile_size"])
    tiles, images = {}, {}
    for key, lst in meta["tiles"].items():
        z = int(key)
        tiles[z] = np.asarray(lst, dtype=np.uint32).reshape(-1, 2)
        images[z] = np.zeros((len(lst), T, T, 4), dtype=np.uint8)
        for k, (x, y) in enumerate(lst):
            with open(os.path.join(directory, str(z), str(x), f"{y}.png"), "rb") as f:
                images[z][k] = png_decode(f.read())
    return dict(scheme=meta["scheme"], format=meta["format"], tile_size=T, minzoom=int(meta["minzoom"]), maxzoom=int(meta["maxzoom"]),
                bounds=[float(v) for v in meta["bounds"]], tiles=tiles, images=images)


class MapTiles:
    """One pcv_maptiles: ECEF points in (add_points / add_query_batch), finish, optionally build_parents, then the tiles of
    every built zoom — ascending by (x, y) — as arrays, as PNG files in memory or as a z/x/y directory."""

    def __init__(self, ctx, handle, params):
        self.ctx, self.lib, self.handle, self.params = ctx, ctx.lib, handle, params
        self.zoom, self.tile_size = int(params.zoom), 256
        ctx._children.add(self)

    def _live(self):
        if not self.handle or not self.ctx.handle:
            raise L.PcvError(L.PCV_E_INVALID, "the map-tile layer was freed")

    def add_points(self, x, y, z, rgb):
        """f64 ECEF planes and 3-byte colours, numpy arrays or torch device tensors (pcv_maptiles_add_points)."""
        self._live()
        bufs = [_Buf(x, np.float64, "x"), _Buf(y, np.float64, "y"), _Buf(z, np.float64, "z"), _Buf(rgb, np.uint8, "rgb")]
        n = bufs[0].size
        if bufs[1].size != n or bufs[2].size != n or bufs[3].size != 3 * n:
            raise ValueError("x, y, z of n points and rgb of 3 n bytes")
        if len({b.device for b in bufs}) != 1:
            raise ValueError("all point arrays must live in the same memory space")
        if bufs[0].device:
            self.ctx.wait_torch()
        self.ctx._check(self.lib.pcv_maptiles_add_points(self.handle, n, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr,
                                                         L.MEM_DEVICE if bufs[0].device else L.MEM_HOST))
        return self

    def add_query_batch(self, batch, shape=None, first_segment=0, num_segments=None):
        """The points of a QueryBatch or S2QueryBatch: of shape `shape`, or of a segment range (default: all), pulled through
        a bounded staging buffer on the device (pcv_maptiles_add_query_batch / pcv_maptiles_add_s2_query)."""
        self._live()
        batch._live()
        first, num = batch._ply_range(shape, first_segment, num_segments)
        fn = self.lib.pcv_maptiles_add_s2_query if isinstance(batch, S2QueryBatch) else self.lib.pcv_maptiles_add_query_batch
        self.ctx._check(fn(self.handle, batch.handle, first, num))
        return self

    def finish(self):
        self._live()
        self.ctx._check(self.lib.pcv_maptiles_finish(self.handle))
        return self

    def build_parents(self, min_zoom):
        """The levels zoom - 1 down to min_zoom (pcv_maptiles_build_parents)."""
        self._live()
        self.ctx._check(self.lib.pcv_maptiles_build_parents(self.handle, int(min_zoom)))
        return self

    def info(self):
        self._live()
        inf = L.MapTilesInfo()
        self.ctx._check(self.lib.pcv_maptiles_info_get(self.handle, C.byref(inf)))
        lo = inf.min_zoom if inf.finished else inf.zoom
        return dict(points_added=inf.points_added, dropped=inf.dropped, drawn=inf.drawn, pool_bytes=inf.pool_bytes, zoom=inf.zoom,
                    min_zoom=inf.min_zoom, finished=bool(inf.finished), tiles={z: int(inf.tiles[z]) for z in range(lo, inf.zoom + 1)})

    def _zoom(self, zoom):
        return self.zoom if zoom is None else int(zoom)

    def _count(self, zoom):
        n = C.c_uint64()
        self.ctx._check(self.lib.pcv_maptiles_tiles(self.handle, zoom, 0, None, C.byref(n)))
        return n.value

    def tiles(self, zoom=None):
        """Tile positions (x, y) of `zoom` (default: the maximum), uint32 [n, 2], ascending by (x, y)."""
        self._live()
        zoom = self._zoom(zoom)
        n = self._count(zoom)
        out = np.zeros((n, 2), dtype=np.uint32)
        self.ctx._check(self.lib.pcv_maptiles_tiles(self.handle, zoom, n, out.ctypes.data, None))
        return out

    def _range(self, zoom, first, count):
        n = self._count(zoom)
        first = int(first)
        num = max(n - first, 0) if count is None else int(count)
        if not (0 <= first <= n and 0 <= num <= n - first):
            raise L.PcvError(L.PCV_E_INVALID, f"tile range past the end: tiles [{first}, {first + num}) of {n}")
        return first, num

    def _plane(self, call, first, num, tail, dtype, device):
        if device:
            import torch
            out = torch.empty((num, 256, 256) + tail, dtype=getattr(torch, np.dtype(dtype).name), device=f"cuda:{self.ctx.device}")
            self.ctx.wait_torch()
            ptr, mem = out.data_ptr(), L.MEM_DEVICE
        else:
            out = np.zeros((num, 256, 256) + tail, dtype=dtype)
            ptr, mem = out.ctypes.data, L.MEM_HOST
        if num:
            self.ctx._check(call(first, num, mem, ptr))
        return out

    def images(self, zoom=None, first=0, count=None, device=False):
        """uint8 [n, 256, 256, 4]: the RGBA images of tiles [first, first + count) of `zoom`; row 0 is north."""
        self._live()
        zoom = self._zoom(zoom)
        first, num = self._range(zoom, first, count)
        return self._plane(lambda f, c, mem, ptr: self.lib.pcv_maptiles_images(self.handle, zoom, f, c, mem, ptr), first, num, (4,), np.uint8, device)

    def counts(self, first=0, count=None, device=False):
        """[n, 256, 256] points per pixel of the tiles of the maximum zoom (uint32; int32 bits on the device)."""
        self._live()
        first, num = self._range(self.zoom, first, count)
        return self._plane(lambda f, c, mem, ptr: self.lib.pcv_maptiles_counts(self.handle, f, c, mem, ptr), first, num, (),
                           np.int32 if device else np.uint32, device)

    def tile_pngs(self, zoom=None, first=0, count=None, png="stored"):
        """The complete PNG files of tiles [first, first + count) of `zoom` as a list of bytes (pcv_maptiles_tile_pngs)."""
        self._live()
        zoom, mode = self._zoom(zoom), _png_mode(png)
        first, num = self._range(zoom, first, count)
        offsets = np.zeros(num + 1, dtype=np.uint64)
        cap = num * int(self.lib.pcv_xray_png_bound(256, 256, mode))
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.ctx._check(self.lib.pcv_maptiles_tile_pngs(self.handle, zoom, first, num, mode, cap, out.ctypes.data, offsets.ctypes.data))
        return _split_files(out, offsets)

    def write(self, directory, png="stored"):
        """<directory>/<z>/<x>/<y>.png of every built zoom and <directory>/tiles.json (pcv_maptiles_write_dir)."""
        self._live()
        self.ctx._check(self.lib.pcv_maptiles_write_dir(self.handle, os.fsencode(str(directory)), _png_mode(png)))

    def free(self):
        if self.handle and self.ctx.handle:
            self.lib.pcv_maptiles_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _cloud_map_tiles(cloud, shapes, zoom, min_zoom, params, into=None):
    """The points `shapes` select from an octree or an S2 cloud (None: all) into `into`, or into a new finished MapTiles."""
    ctx = cloud.ctx
    own = shapes is None
    if own:
        shapes = ctx.shapes([("all",)])
    batch = m = None
    try:
        batch = cloud.query_batch(shapes)
        m = into if into is not None else ctx.map_tiles_begin(zoom, **params)
        m.add_query_batch(batch)
        if into is not None:
            return m
        m.finish()
        return m if min_zoom is None else m.build_parents(min_zoom)
    except Exception:
        if m is not None and into is None:
            m.free()
        raise
    finally:
        if batch is not None:
            batch.free()
        if own:
            shapes.free()


def build_map_tiles(cloud_dir, out_dir, zoom, min_zoom=None, png="stored", ctx=None, **params):
    """A z/x/y map-tile directory from an ECEF cloud directory, or from a list of them: the kind of the first one (cloud_kind)
    decides, every directory is opened as that kind, all their points go into one layer at `zoom`, the parents are built down
    to `min_zoom` (None: none) and the pyramid is written to out_dir. ctx: None = the default context; params:
    map_tiles_params' arguments. Returns the finished MapTiles."""
    ctx = ctx if ctx is not None else default_context()
    locations = [cloud_dir] if isinstance(cloud_dir, (str, os.PathLike)) else list(cloud_dir)
    if not locations:
        raise ValueError("No locations specified for point cloud client.")
    map_tiles_check_params(zoom, min_zoom, **params)
    _png_mode(png)  # an unknown mode is refused before any work
    opener = ctx.s2_open if cloud_kind(locations[0]) == "s2" else ctx.open_dir
    clouds = [opener(d) for d in locations]
    m = None
    try:
        m = ctx.map_tiles_begin(zoom, **params)
        for c in clouds:
            _cloud_map_tiles(c, None, zoom, None, params, into=m)
        m.finish()
        if min_zoom is not None:
            m.build_parents(min_zoom)
        m.write(out_dir, png=png)
        return m
    except Exception:
        if m is not None:
            m.free()
        raise
    finally:
        for c in clouds:
            c.free()


def tiles3d_params(error_factor=None, transform=None, intensity=False, position_mode="auto", chunk_bytes=None):
    """pcv_tiles3d_params. error_factor: None = 0.0625; transform: 16 doubles, column-major (or a 4 x 4 array, whose transpose's
    rows they are), None = none; position_mode: "auto", "quantized", "float" or the PCV_TILES3D_POS_* number; chunk_bytes: None or
    0 = 256 MiB."""
    pr = L.Tiles3dParams()
    pr.error_factor = L.TILES3D_DEFAULT_ERROR_FACTOR if error_factor is None else float(error_factor)
    if transform is not None:
        m = np.asarray(transform, dtype=np.float64)
        m = m.T.ravel() if m.shape == (4, 4) else m.ravel()
        if m.size != 16:
            raise ValueError("transform: 16 doubles, column-major, or a 4 x 4 array")
        pr.transform[:] = [float(v) for v in m]
    pr.flags = L.TILES3D_INTENSITY if intensity else 0
    if isinstance(position_mode, str):
        if position_mode not in L.TILES3D_POS_NAMES:
            raise ValueError(f"position_mode: one of {L.TILES3D_POS_NAMES}")
        position_mode = L.TILES3D_POS_NAMES.index(position_mode)
    pr.position_mode = int(position_mode)
    pr.chunk_bytes = int(chunk_bytes or 0)
    return pr


def tiles3d_check_params(**params):
    """pcv_tiles3d_check_params_host: raises PcvError with the rule that is broken. params: tiles3d_params' arguments, or
    params=a Tiles3dParams."""
    pr = params["params"] if "params" in params else tiles3d_params(**params)
    _host_check(L.load_library().pcv_tiles3d_check_params_host(C.byref(pr)), "pcv_tiles3d_check_params_host")


def _node_info(node):
    """A NodeInfo from a NodeInfo or a dict(id=(high, low) | id_high, id_low, num_points, level, encoding, cube_min, cube_edge)."""
    if isinstance(node, L.NodeInfo):
        return node
    nd = L.NodeInfo()
    hi, lo = node["id"] if "id" in node else (node["id_high"], node["id_low"])
    nd.id_high, nd.id_low, nd.num_points = int(hi), int(lo), int(node["num_points"])
    nd.level = int(node["level"]) if "level" in node else int(hi) >> 56
    nd.encoding = int(node.get("encoding", L.ENC_FLOAT32))
    nd.cube_min[:] = [float(v) for v in node["cube_min"]]
    nd.cube_edge = float(node["cube_edge"])
    return nd


def tiles3d_rtc(node):
    """RTC_CENTER of a node's tile (pcv_tiles3d_rtc_host): (double)(float)(cube_min + cube_edge / 2) per axis."""
    out = (C.c_double * 3)()
    _host_check(L.load_library().pcv_tiles3d_rtc_host(C.byref(_node_info(node)), C.byref(out)), "pcv_tiles3d_rtc_host")
    return np.array(out[:])


def tiles3d_tile_host(node, xyz, rgb, intensity=None, with_plan=False, **params):
    """One complete .pnts file from a node's record and its bytes on the host (pcv_tiles3d_tile_host), the device's twin.
    intensity: the node's .intensity bytes (or float32 array); params: tiles3d_params' arguments, where intensity=True is implied
    by passing the bytes. with_plan: also the file's plan as a dict."""
    nd = _node_info(node)
    if intensity is not None:
        params = dict(params, intensity=params.get("intensity", True))
    pr = params["params"] if "params" in params else tiles3d_params(**params)
    bufs = [np.frombuffer(bytes(b), dtype=np.uint8) if isinstance(b, (bytes, bytearray, memoryview)) else np.ascontiguousarray(b).view(np.uint8).ravel()
            for b in (xyz, rgb)]
    ib = None
    if intensity is not None:
        ib = (np.frombuffer(bytes(intensity), dtype=np.uint8) if isinstance(intensity, (bytes, bytearray, memoryview))
              else np.ascontiguousarray(intensity, dtype=np.float32).view(np.uint8).ravel())
    n = int(nd.num_points)
    bpc = {L.ENC_UINT8: 1, L.ENC_UINT16: 2, L.ENC_FLOAT32: 4, L.ENC_FLOAT64: 8}.get(int(nd.encoding), 0)
    if bufs[0].size != 3 * n * bpc or bufs[1].size != 3 * n or (ib is not None and ib.size != 4 * n):
        raise ValueError("the node's bytes do not match its num_points and encoding")
    lib, ln, tile = L.load_library(), C.c_uint64(), L.Tiles3dTile()
    ip = ib.ctypes.data if ib is not None else None
    _host_check(lib.pcv_tiles3d_tile_host(C.byref(nd), C.byref(pr), bufs[0].ctypes.data, bufs[1].ctypes.data, ip, None, 0, C.byref(ln), C.byref(tile)),
                "pcv_tiles3d_tile_host")
    out = np.zeros(ln.value, dtype=np.uint8)
    _host_check(lib.pcv_tiles3d_tile_host(C.byref(nd), C.byref(pr), bufs[0].ctypes.data, bufs[1].ctypes.data, ip, out.ctypes.data, out.size, C.byref(ln),
                                          None), "pcv_tiles3d_tile_host")
    return (out.tobytes(), _tiles3d_tile(tile)) if with_plan else out.tobytes()


def tiles3d_tileset_json(nodes, **params):
    """The text of tileset.json for a node table (pcv_tiles3d_tileset_json_host): NodeInfo records or the dicts of _node_info,
    ascending by (level, index). params: tiles3d_params' arguments."""
    pr = params["params"] if "params" in params else tiles3d_params(**params)
    arr = (L.NodeInfo * max(1, len(nodes)))()
    for k, node in enumerate(nodes):
        arr[k] = _node_info(node)
    lib, n = L.load_library(), C.c_uint64()
    _host_check(lib.pcv_tiles3d_tileset_json_host(arr, len(nodes), C.byref(pr), None, 0, C.byref(n)), "pcv_tiles3d_tileset_json_host")
    buf = C.create_string_buffer(n.value + 1)
    _host_check(lib.pcv_tiles3d_tileset_json_host(arr, len(nodes), C.byref(pr), buf, n.value, C.byref(n)), "pcv_tiles3d_tileset_json_host")
    return buf.raw[:n.value].decode()


def _tiles3d_tile(t):
    return dict(node=int(t.node), num_points=int(t.num_points), mode=L.TILES3D_POS_NAMES[t.mode], file_bytes=int(t.file_bytes),
                feature_json_offset=int(t.feature_json_offset), feature_binary_offset=int(t.feature_binary_offset),
                batch_json_offset=int(t.batch_json_offset), batch_binary_offset=int(t.batch_binary_offset))


class Tiles3D:
    """One pcv_tiles3d: the plan of an octree as a 3D Tiles 1.0 tileset. The .pnts files are packed on the device from the
    node blobs the octree holds there, into memory (tile_files) or into a directory (write)."""

    def __init__(self, tree, handle, params):
        self.tree, self.ctx, self.lib, self.handle, self.params = tree, tree.ctx, tree.lib, handle, params
        self.ctx._children.add(self)

    def _live(self):
        if not self.handle or not self.ctx.handle or not self.tree.handle:
            raise L.PcvError(L.PCV_E_INVALID, "the tileset plan or its octree was freed")

    @property
    def info(self):
        self._live()
        inf = L.Tiles3dInfo()
        self.ctx._check(self.lib.pcv_tiles3d_info_get(self.handle, C.byref(inf)))
        return dict(tiles=int(inf.tiles), content_tiles=int(inf.content_tiles), points=int(inf.points),
                    total_file_bytes=int(inf.total_file_bytes), chunk_points=int(inf.chunk_points))

    def tiles(self):
        """The content tiles in node-table order: dicts of node (index into the octree's node table), num_points, mode
        ("quantized" / "float"), file_bytes and the four section offsets."""
        self._live()
        n = C.c_uint64()
        self.ctx._check(self.lib.pcv_tiles3d_tiles(self.handle, 0, None, C.byref(n)))
        arr = (L.Tiles3dTile * max(1, n.value))()
        self.ctx._check(self.lib.pcv_tiles3d_tiles(self.handle, n.value, arr, None))
        return [_tiles3d_tile(arr[k]) for k in range(n.value)]

    def tile_files(self, first=0, count=None, device=False):
        """The complete .pnts files of content tiles [first, first + count) (pcv_tiles3d_tile_files): a list of bytes, or with
        device=True (a uint8 torch tensor on the device holding them back to back, uint64 offsets [count + 1])."""
        self._live()
        total = self.info["content_tiles"]
        first = int(first)
        num = max(total - first, 0) if count is None else int(count)
        if not (0 <= first <= total and 0 <= num <= total - first):
            raise L.PcvError(L.PCV_E_INVALID, f"tile range past the end: tiles [{first}, {first + num}) of {total}")
        offsets = np.zeros(num + 1, dtype=np.uint64)
        self.ctx._check(self.lib.pcv_tiles3d_tile_files(self.handle, first, num, L.MEM_HOST, 0, None, offsets.ctypes.data))
        cap = int(offsets[-1])
        if device:
            import torch
            out = torch.empty(max(cap, 1), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
            self.ctx.wait_torch()
            self.ctx._check(self.lib.pcv_tiles3d_tile_files(self.handle, first, num, L.MEM_DEVICE, cap, out.data_ptr(), offsets.ctypes.data))
            return out[:cap], offsets
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        self.ctx._check(self.lib.pcv_tiles3d_tile_files(self.handle, first, num, L.MEM_HOST, cap, out.ctypes.data, offsets.ctypes.data))
        return _split_files(out, offsets)

    def tileset_json(self):
        self._live()
        n = C.c_uint64()
        self.ctx._check(self.lib.pcv_tiles3d_tileset_json(self.handle, None, 0, C.byref(n)))
        buf = C.create_string_buffer(n.value + 1)
        self.ctx._check(self.lib.pcv_tiles3d_tileset_json(self.handle, buf, n.value, C.byref(n)))
        return buf.raw[:n.value].decode()

    def write(self, directory):
        """<directory>/<NodeId>.pnts of every content tile, then <directory>/tileset.json (pcv_tiles3d_write_dir)."""
        self._live()
        self.ctx._check(self.lib.pcv_tiles3d_write_dir(self.handle, os.fsencode(str(directory))))

    def free(self):
        if self.handle and self.ctx.handle:
            self.lib.pcv_tiles3d_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def build_3d_tiles(octree_dir, out_dir, ctx=None, **params):
    """A 3D Tiles directory (tileset.json and one .pnts per node that holds points) from an octree directory. ctx: None = the
    default context; params: tiles3d_params' arguments. Returns the tileset's info."""
    ctx = ctx if ctx is not None else default_context()
    tiles3d_check_params(**params)
    tree = ctx.open_dir(octree_dir)
    t = None
    try:
        t = tree.tiles3d(**params)
        t.write(out_dir)
        return t.info
    finally:
        if t is not None:
            t.free()
        tree.free()


def read_3d_tiles(directory):
    """A 3D Tiles directory as this library writes it, in pure Python: walks tileset.json and returns one dict per tile in
    document order: uri (None without content), box (12 doubles), geometric_error, depth, parent (index into the list, -1 for
    the root), and for a content tile positions (float64 [n, 3]: rc + offset + q * scale / 65535, or rc + (double)f), rgb
    (uint8 [n, 3]), intensity (float32 [n] or None), quantized (bool)."""
    import json
    import struct
    directory = str(directory)
    with open(os.path.join(directory, "tileset.json")) as f:
        doc = json.load(f)
    out = []

    def walk(t, parent, depth):
        rec = dict(uri=None, box=[float(v) for v in t["boundingVolume"]["box"]], geometric_error=float(t["geometricError"]), depth=depth,
                   parent=parent, positions=None, rgb=None, intensity=None, quantized=None)
        me = len(out)
        out.append(rec)
        if "content" in t:
            rec["uri"] = t["content"]["uri"]
            with open(os.path.join(directory, rec["uri"]), "rb") as f:
                data = f.read()
            magic, version, total, fj, fb, bj, bb = struct.unpack_from("<4sIIIIII", data, 0)
            if magic != b"pnts" or version != 1 or total != len(data) or 28 + fj + fb + bj + bb != total:
                raise ValueError(f"{rec['uri']}: not a .pnts file of version 1")
            ft = json.loads(data[28:28 + fj].decode())
            n, fbin = int(ft["POINTS_LENGTH"]), 28 + fj
            rc = np.array(ft["RTC_CENTER"], dtype=np.float64)
            if "POSITION_QUANTIZED" in ft:
                q = np.frombuffer(data, dtype="<u2", count=3 * n, offset=fbin + ft["POSITION_QUANTIZED"]["byteOffset"]).reshape(n, 3)
                off, scale = np.array(ft["QUANTIZED_VOLUME_OFFSET"], dtype=np.float64), np.array(ft["QUANTIZED_VOLUME_SCALE"], dtype=np.float64)
                rec["positions"], rec["quantized"] = rc + off + q.astype(np.float64) * scale / 65535.0, True
            else:
                p = np.frombuffer(data, dtype="<f4", count=3 * n, offset=fbin + ft["POSITION"]["byteOffset"]).reshape(n, 3)
                rec["positions"], rec["quantized"] = rc + p.astype(np.float64), False
            rec["rgb"] = np.frombuffer(data, dtype=np.uint8, count=3 * n, offset=fbin + ft["RGB"]["byteOffset"]).reshape(n, 3).copy()
            if bj:
                bt = json.loads(data[fbin + fb:fbin + fb + bj].decode())
                rec["intensity"] = np.frombuffer(data, dtype="<f4", count=n, offset=fbin + fb + bj + bt["INTENSITY"]["byteOffset"]).copy()
        for c in t.get("children", []):
            walk(c, me, depth + 1)

    walk(doc["root"], -1, 0)
    return out


def cloud_kind(directory):
    """"octree" or "s2": how PointCloudClientBuilder::build (point_cloud_client/src/lib.rs:107-132) would open this
    directory, by its meta.pb (pcv_cloud_kind; host only). A missing or unreadable meta.pb raises PcvError (PCV_E_IO)."""
    kind = C.c_int()
    _host_check(L.load_library().pcv_cloud_kind(os.fsencode(str(directory)), C.byref(kind)), "pcv_cloud_kind")
    return "s2" if kind.value == L.CLOUD_S2 else "octree"


def build_xray_quadtree(ctx, point_cloud_locations, output_directory, tile_size_px=256, pixel_size_m=None, strategy="xray",
                        query_from_global=None, intensity_interval=None, background="white", root_node_id="r",
                        max_workspace_bytes=None, min_intensity=0.0, max_intensity=1.0, binning=None, png="stored",
                        filter_intervals=None):
    """The reference's build_xray_quadtree binary over directories: the kind of the first one (cloud_kind) decides, every
    directory is opened as that kind (one of the other kind fails with the opener's own message), leaves and parents are
    built on the device and the quadtree is written to output_directory. Over S2 directories, binning takes any scalar
    attribute and filter_intervals = {name: (lo, hi)} is --filter-interval. Returns the XrayTiles."""
    locations = list(point_cloud_locations)
    if not locations:
        raise ValueError("No locations specified for point cloud client.")
    opener = ctx.s2_open if cloud_kind(locations[0]) == "s2" else ctx.open_dir
    clouds = [opener(d) for d in locations]
    try:
        return ctx.xray_quadtree(clouds, tile_size_px, pixel_size_m, strategy, query_from_global, intensity_interval, background,
                                 root_node_id, max_workspace_bytes, min_intensity, max_intensity, binning,
                                 output_directory=output_directory, png=png, filter_intervals=filter_intervals)
    finally:
        for c in clouds:
            c.free()


def build_s2_cells(output_directory, points, split_level=20, ctx=None, open_mode="truncate", flush_points=None):
    """An S2 cell cloud directory of ECEF points, as S2Splitter (src/read_write/s2.rs) writes it: `points` =
    dict(x=, y=, z=, color=[, intensity=]), one batch, split and written whole — or, like the reference, an ITERATOR OF
    BATCHES (PointsBatch dicts with position=, or SoA dicts) through a directory stream (Context.s2_stream): device memory
    stays O(flush_points), the result is the same directory. open_mode "append" adds to the S2 directory that is there (always
    through the stream). Returns the S2Cloud."""
    ctx = ctx or default_context()
    if isinstance(points, dict) and open_mode == "truncate" and flush_points is None:
        cloud = ctx.s2_split(points, split_level)
        cloud.write(output_directory)
        return cloud
    with ctx.s2_stream(split_level, output_directory, open_mode, flush_points) as stream:
        for batch in ([points] if isinstance(points, dict) else points):
            stream.append(batch)
        return stream.finish()


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def build_octree(output_directory, resolution, bounding_box, points, attributes=("color",), ctx=None,
                 max_points_per_node=0, max_points_per_pass=None):
    """Drop-in for reference `build_octree` (generation.rs:289-295): builds on the GPU and writes the
    reference's directory layout. `points` = dict(x=, y=, z=, color=, intensity=optional) — or, like the reference, an
    ITERATOR OF BATCHES, each dict(position=(n, 3) f64, color=(n, 3) u8[, intensity=(n,) f32]) (PointsBatch,
    src/lib.rs:102-107): the batches are streamed to the device one at a time (pcv_ingest_*), host memory stays O(batch).
    An iterator with `num_points` (NumberOfPoints, src/lib.rs:56-58) sizes the device arrays up front.
    max_points_per_pass: None = the in-core build above. An integer (0 = derived from free device memory) takes the
    out-of-core build (pcv_ooc_*) for clouds larger than the device: the batches wait in host memory, the tree is built
    partition by partition straight into the directory, and the build's statistics (a dict) are returned instead of an
    OctreeResult. The bounding box is required then."""
    attributes = tuple(attributes)
    if "color" not in attributes:
        raise ValueError("the octree format requires the 'color' attribute (on_disk.rs:20-22)")
    for a in attributes:
        if a not in ("color", "intensity"):
            raise ValueError(f"unsupported attribute {a!r} (octree/mod.rs:62-74 implies color and intensity)")
    ctx = ctx or default_context()
    if max_points_per_pass is not None:
        want_intensity = "intensity" in attributes
        if isinstance(points, dict):
            pos = np.stack([np.asarray(points["x"]), np.asarray(points["y"]), np.asarray(points["z"])], axis=1)
            one = dict(position=pos, color=points["color"], intensity=points.get("intensity"))
            points = [one]
        ooc = ctx.out_of_core(resolution, bounding_box, want_intensity, max_points_per_pass, max_points_per_node)
        try:
            for batch in points:
                if want_intensity and batch.get("intensity") is None:
                    raise ValueError("attribute 'intensity' requested but not present in the input")
                ooc.append(batch["position"], batch["color"], batch.get("intensity") if want_intensity else None)
        except BaseException:
            ooc.abort()
            raise
        return ooc.finish(output_directory)
    if not isinstance(points, dict):
        want_intensity = "intensity" in attributes
        hint = getattr(points, "num_points", 0)
        ing = ctx.ingest(hint() if callable(hint) else int(hint or 0), want_intensity)
        try:
            for batch in points:
                if want_intensity and batch.get("intensity") is None:
                    raise ValueError("attribute 'intensity' requested but not present in the input")
                ing.append(batch["position"], batch["color"], batch.get("intensity") if want_intensity else None)
        except BaseException:
            ing.abort()
            raise
        tree = ing.finish(resolution, bounding_box, max_points_per_node)
        tree.write_dir(output_directory)
        return tree
    inten = points.get("intensity") if "intensity" in attributes else None
    if "intensity" in attributes and inten is None:
        raise ValueError("attribute 'intensity' requested but not present in the input")
    tree = ctx.build(resolution, bounding_box, points["x"], points["y"], points["z"], points["color"], inten,
                     max_points_per_node)
    tree.write_dir(output_directory)
    return tree
