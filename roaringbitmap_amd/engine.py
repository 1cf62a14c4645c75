"""Device-resident session API (rbg_ctx_*): one HIP stream + workspace per context.

Used by bench.py (HIP-event timing on `stream_ptr`) and by multi-GPU sharding
(`fetch_shard`).  All op calls enqueue asynchronously; `sync()` waits.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import as_u32, call_bytes, check, ids_array, is_torch, lib, take
from .roaring import RoaringBitmap

SYNTH_C2, SYNTH_C3_UNIFORM, SYNTH_C3_CLUSTERED, SYNTH_C4_PAIRS, SYNTH_C5_BSI = 0, 1, 2, 3, 4


def _dptr(t):
    """the device pointer of a tensor, null for an empty one"""
    return ctypes.c_void_p(t.data_ptr()) if t.numel() else None


def _index_call(f, *args):
    """f(*args, &batch, out3): a session call that makes a bit-sliced index -> (batch, nbits, minValue, maxValue)"""
    out = ctypes.c_int32()
    out3 = (ctypes.c_int32 * 3)()
    check(f(*args, ctypes.byref(out), out3))
    return out.value, int(out3[0]), int(out3[1]), int(out3[2])


def synth_key_bytes(kind, seed, n) -> np.ndarray:
    """Per-key algorithmic input bytes of a synthetic C3 workload (host, for key-range partitioning)."""
    out = np.zeros(65536, dtype=np.uint64)
    check(lib().rbg_synth_key_bytes(int(kind), int(seed), int(n),
                                    out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))))
    return out


class Engine:
    def __init__(self, device=0):
        self._ctx = ctypes.c_void_p()
        check(lib().rbg_ctx_create(int(device), ctypes.byref(self._ctx)))
        self.device = device
        self._bsi_target = None  # device tensor the BSI sum kernels write into (bsi_sums_target)

    def close(self):
        if self._ctx:
            lib().rbg_ctx_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()
        self._bsi_target = None  # the BSI sums target is released with the context that wrote it

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream_ptr(self) -> int:
        return lib().rbg_ctx_stream(self._ctx)

    def sync(self):
        check(lib().rbg_ctx_sync(self._ctx))

    def profile(self, max_ops, compute_only=False):
        """Enable HIP-event phase timing for the next `max_ops` ops (0 disables); compute_only: two events
        per op around the container compute kernel (only compute_ms is read)."""
        f = lib().rbg_ctx_profile_compute if compute_only else lib().rbg_ctx_profile
        check(f(self._ctx, int(max_ops)))

    def profile_read(self):
        """-> (n_ops, [plan_ms, compute_ms, assemble_ms]) summed over the recorded ops."""
        ms = (ctypes.c_double * 3)()
        n = ctypes.c_int()
        check(lib().rbg_ctx_profile_read(self._ctx, ms, ctypes.byref(n)))
        return n.value, list(ms)

    def profile_bytes(self) -> int:
        """Bytes the early-exit wide AND (workShyAnd) read since profiling was enabled."""
        v = ctypes.c_int64()
        check(lib().rbg_ctx_profile_bytes(self._ctx, ctypes.byref(v)))
        return v.value

    # ---- batches ------------------------------------------------------------
    def load(self, bitmaps, packed=False) -> int:
        """Upload + device decode of serialized bitmaps as one key-major batch.  packed: for a batch
        that feeds wide ops -- a batch of arrays alone keeps the portable format's packed array
        payloads (rbg_ctx_load_packed), the wide kernels' fastest layout."""
        bufs = [b.serialize() if isinstance(b, RoaringBitmap) else bytes(b) for b in bitmaps]
        arr, lens = _lib.buf_array(bufs)
        out = ctypes.c_int32()
        f = lib().rbg_ctx_load_packed if packed else lib().rbg_ctx_load
        check(f(self._ctx, arr, lens, len(bufs), ctypes.byref(out)))
        return out.value

    def load_pair(self, *bitmaps):
        """Upload several serialized bitmaps at once, each decoded into a batch of its own
        (rbg_ctx_load_separate): the operands of pairwise ops.  -> list of batch ids."""
        bufs = [b.serialize() if isinstance(b, RoaringBitmap) else bytes(b) for b in bitmaps]
        arr, lens = _lib.buf_array(bufs)
        ids = (ctypes.c_int32 * max(len(bufs), 1))()
        check(lib().rbg_ctx_load_separate(self._ctx, arr, lens, len(bufs), ids))
        return list(ids)[:len(bufs)]

    def synth(self, kind, seed, n=0, key_lo=0, key_hi=65536) -> int:
        out = ctypes.c_int32()
        check(lib().rbg_ctx_synth(self._ctx, int(kind), int(seed), int(n), int(key_lo), int(key_hi),
                                  ctypes.byref(out)))
        return out.value

    def release(self, batch):
        check(lib().rbg_ctx_release(self._ctx, int(batch)))

    def batch_stats(self, batch) -> dict:
        s = (ctypes.c_int64 * 8)()
        check(lib().rbg_ctx_batch_stats(self._ctx, int(batch), s))
        keys = ["bitmaps", "containers", "array", "bitmap", "run", "payload_bytes", "cardinality", "serialized_bytes"]
        return dict(zip(keys, list(s)))

    def batch_fetch(self, batch, i=0) -> RoaringBitmap:
        return RoaringBitmap(call_bytes(lib().rbg_ctx_batch_fetch, self._ctx, int(batch), int(i)))

    def batch_fetch_range(self, batch, first=0, count=None) -> list:
        """Bitmaps [first, first + count) of a batch (default: all), one device gather + one copy."""
        if count is None:
            count = self.batch_stats(batch)["bitmaps"] - first
        outs = (_lib.rbg_buffer * max(count, 1))()
        check(lib().rbg_ctx_batch_fetch_range(self._ctx, int(batch), int(first), int(count), outs))
        return [RoaringBitmap(take(outs[k])) for k in range(count)]

    # ---- ops (asynchronous) -------------------------------------------------------
    def pairwise(self, op, a, b, ia=0, ib=0, key_lo=0, key_hi=65536):
        """A pairwise op; key_lo / key_hi restrict it to one key-range shard (shard.py assembles shards)."""
        if key_lo == 0 and key_hi == 65536:
            check(lib().rbg_ctx_pairwise(self._ctx, _lib.OP[op], int(a), int(ia), int(b), int(ib)))
        else:
            check(lib().rbg_ctx_pairwise_range(self._ctx, _lib.OP[op], int(a), int(ia), int(b), int(ib), int(key_lo),
                                               int(key_hi)))

    def ornot(self, a, b, range_end, inplace=False, buffer=False, ia=0, ib=0):
        """RoaringBitmap.orNot(x1, x2, rangeEnd) (inplace: x1.orNot(x2, rangeEnd); buffer: the buffer
        package's) of two resident bitmaps; the result pending like pairwise's (rbg_ctx_ornot)."""
        flags = (_lib.RBG_ORNOT_INPLACE if inplace else 0) | (_lib.RBG_ORNOT_BUFFER if buffer else 0)
        check(lib().rbg_ctx_ornot(self._ctx, int(a), int(ia), int(b), int(ib), int(range_end), flags))

    def range_mut(self, op, a, range_start, range_end, buffer=False, ia=0):
        """static RoaringBitmap.add / remove / flip(rb, start, end) ("add" / "remove" / "flip"; buffer:
        MutableRoaringBitmap's) of a resident bitmap; the result pending like pairwise's (rbg_ctx_range_mut)."""
        code = _lib.RMUT_OP[op] | (_lib.RBG_RMUT_BUFFER if buffer else 0)
        check(lib().rbg_ctx_range_mut(self._ctx, code, int(a), int(ia), int(range_start), int(range_end)))

    def add_offset(self, a, offset, ia=0):
        """RoaringBitmap.addOffset(x, offset) of a resident bitmap; the result pending like pairwise's
        (rbg_ctx_add_offset)."""
        check(lib().rbg_ctx_add_offset(self._ctx, int(a), int(ia), int(offset)))

    def pairwise_serialized(self, op, a, b, ia=0, ib=0):
        """pairwise(op) + serialize() in one call (rbg_ctx_pairwise_serialized): the same launches and the
        same bytes as the two calls."""
        check(lib().rbg_ctx_pairwise_serialized(self._ctx, _lib.OP[op], int(a), int(ia), int(b), int(ib)))

    def and_cardinality(self, a, b, ia=0, ib=0):
        check(lib().rbg_ctx_pairwise_card(self._ctx, 0, int(a), int(ia), int(b), int(ib)))

    def wide(self, op, batch, key_lo=0, key_hi=65536, ids=None):
        check(lib().rbg_ctx_wide(self._ctx, _lib.WIDE_OP[op], int(batch), int(key_lo), int(key_hi), ids_array(ids)))

    def wide_start(self, op, batch, key_lo, key_hi, start_bm, ids=None):
        """wide op whose naive_and chain starts from input `start_bm` (key-range shards)."""
        check(lib().rbg_ctx_wide_start(self._ctx, _lib.WIDE_OP[op], int(batch), int(key_lo), int(key_hi),
                                       ids_array(ids), int(start_bm)))

    def pair_bytes(self, batch):
        """(matched payload + descriptors, all payload + descriptors) of a batch of pairs (C4)."""
        out = (ctypes.c_int64 * 2)()
        check(lib().rbg_ctx_pair_bytes(self._ctx, int(batch), out))
        return int(out[0]), int(out[1])

    def run_optimize(self, batch, answers=True):
        """RoaringBitmap.runOptimize (RB/RoaringBitmap.java:2764-2774) of every bitmap of a batch, on the
        device -> (new batch id, [runOptimize's boolean per bitmap]).  The booleans need a read-back
        (synchronous); answers=False returns (id, None) with nothing read back: the new batch's
        statistics stay on the device until a host-side use needs them."""
        out = ctypes.c_int32()
        if not answers:
            check(lib().rbg_ctx_run_optimize(self._ctx, int(batch), ctypes.byref(out), None))
            return int(out.value), None
        n = self.batch_stats(batch)["bitmaps"]
        ans = (ctypes.c_uint8 * max(n, 1))()
        check(lib().rbg_ctx_run_optimize(self._ctx, int(batch), ctypes.byref(out), ans))
        return int(out.value), [bool(x) for x in ans[:n]]

    def select_range(self, batch, start, end):
        """selectRangeWithoutCopy (RB/RoaringBitmap.java:3160-3214) of every bitmap of a batch, on the device
        -> new batch id (rbg_ctx_select_range)."""
        out = ctypes.c_int32()
        check(lib().rbg_ctx_select_range(self._ctx, int(batch), int(start), int(end), ctypes.byref(out)))
        return int(out.value)

    def batch_minmax(self, batch):
        out = (ctypes.c_int32 * 2)()
        check(lib().rbg_ctx_batch_minmax(self._ctx, int(batch), out))
        return int(out[0]), int(out[1])

    def bsi(self, batch, op, nbits, start, end=0, min_value=0, max_value=0, has_found=False, want_sum=False):
        """RoaringBitmapSliceIndex.compare (op in BitmapSliceIndex.Operation order; 8 = sum alone) over a
        key-major batch [ebM, bA[0..nbits-1], foundSet?]; want_sum fuses sum(result)."""
        code = _lib.bsi_op(op)
        check(lib().rbg_ctx_bsi(self._ctx, int(batch), code, int(nbits), int(bool(has_found)), int(start), int(end),
                                int(min_value), int(max_value), int(bool(want_sum))))

    def bsi_buffer(self, batch, op, nbits, start, end=0, min_value=0, max_value=0, has_found=False):
        """The buffer package's BitSliceIndexBase.compare (bsi/.../bsi/buffer/BitSliceIndexBase.java:422-453;
        op 7 = rangeNEQ called directly) over a key-major batch [ebM, bA[0..nbits-1], foundSet?]."""
        code = _lib.bsi_op(op)
        check(lib().rbg_ctx_bsi_buffer(self._ctx, int(batch), code, int(nbits), int(bool(has_found)), int(start),
                                       int(end), int(min_value), int(max_value)))

    def bsi_sums(self):
        out = (ctypes.c_int64 * 2)()
        check(lib().rbg_ctx_bsi_sums(self._ctx, out))
        return int(out[0]), int(out[1])

    def bsi_sums_device(self, dst):
        """(sum, count) of the last BSI call into a device int64 tensor of two elements, enqueued on
        the engine stream (no host synchronisation)."""
        check(lib().rbg_ctx_bsi_sums_device(self._ctx, ctypes.c_void_p(dst.data_ptr())))

    def bsi_sums_target(self, dst):
        """From now on every BSI sum also writes its (sum, count) into the int64 device tensor `dst`
        (two elements) from the kernel that computes it; None stops it (rbg_ctx_bsi_sums_target).

        The engine keeps a reference to `dst` until it is replaced, cleared with None or the engine is
        closed, so the kernels never write into memory the caller's allocator has handed on."""
        if dst is not None:
            import torch
            if not isinstance(dst, torch.Tensor) or dst.dtype != torch.int64 or not dst.is_contiguous() \
                    or dst.numel() < 2 or dst.device.type != "cuda" or dst.device.index != self.device:
                raise ValueError("bsi_sums_target: a contiguous int64 CUDA tensor of at least 2 elements on "
                                 f"device {self.device} is required")
        check(lib().rbg_ctx_bsi_sums_target(self._ctx, None if dst is None else ctypes.c_void_p(dst.data_ptr())))
        self._bsi_target = dst

    def point_query(self, op, batch, queries, ia=0):
        """n point queries against a resident bitmap (rbg_ctx_point_query): op "rank" (rankLong), "select",
        "contains", "next" (nextValue), "prev" (previousValue); one int64 per query, in query order, -1 where
        there is no such value.  A numpy array (or sequence) of values below 2^32 -> numpy int64 array,
        synchronous.  A torch tensor on this engine's GPU, int64 holding values in [0, 2^32) (torch has no
        arithmetic on uint32; a uint32 tensor is taken as it is; as on the numpy path only the low 32 bits
        of a value are read, so -1 asks for 0xFFFFFFFF) -> torch int64 tensor, enqueued on the
        engine stream through the device entry point with no host synchronisation (but for a batch's first
        query, which builds its rank directory); torch's current stream waits for the result, so work
        enqueued there afterwards may read it."""
        code = _lib.PQ_OP[op] if isinstance(op, str) else int(op)
        if is_torch(queries):
            import torch
            q = self._words("point_query", queries, ("int64", "uint32"), "query tensor")
            out = torch.empty(q.numel(), dtype=torch.int64, device=queries.device)
            if q.numel() == 0:
                return out
            done = self._handshake(queries.device)
            check(lib().rbg_ctx_point_query_device(self._ctx, code, int(batch), int(ia),
                                                   ctypes.c_void_p(q.data_ptr()), q.numel(),
                                                   ctypes.c_void_p(out.data_ptr())))
            done()
            return out
        q = as_u32(queries)
        out = np.empty(q.size, dtype=np.int64)
        check(lib().rbg_ctx_point_query(self._ctx, code, int(batch), int(ia),
                                        q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), q.size,
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def _handshake(self, device):
        """Orders the engine stream after torch's current stream on `device`; returns a function that,
        called after the engine work is enqueued, makes the current stream wait for it.  So tensors made on
        the current stream (a conversion of the input) are ready for the engine's kernels; torch's allocator,
        which orders the reuse of a tensor's memory on the current stream alone, cannot hand that memory out
        while those kernels still use it (the tensors keep no reference to the engine stream, which close()
        destroys); and the outputs are ready for work enqueued on the current stream."""
        import torch
        cur = torch.cuda.current_stream(device)
        es = torch.cuda.ExternalStream(self.stream_ptr, device=device)
        ev = torch.cuda.Event()
        ev.record(cur)
        es.wait_event(ev)

        def done():
            d = torch.cuda.Event()
            d.record(es)
            cur.wait_event(d)
        return done

    def _words(self, what, t, dtypes=("int64", "uint32", "int32"), noun="tensor"):
        """A torch tensor on this engine's GPU as flat contiguous 32-bit words: int64 (the low 32 bits of every
        element, little-endian words) or, as it is, another of `dtypes`."""
        import torch
        if t.device.type != "cuda" or t.device.index != self.device:
            raise ValueError(f"{what}: the {noun} must be on device {self.device}")
        if t.dtype == torch.int64:
            w = t.contiguous().reshape(-1).view(torch.int32)[::2].contiguous()
        elif t.dtype in [getattr(torch, d) for d in dtypes]:
            w = t.contiguous()
        else:
            raise ValueError(f"{what}: an {', '.join(dtypes[:-1])} or {dtypes[-1]} tensor is required")
        return w.reshape(-1)

    def _pairs(self, what, columns, values):
        """The shared front of the calls that take (column, value) pairs -> (done, columns pointer, values
        pointer, n).  Tensors: both must be, of one length, int64 values in [0, 2^31); they are read in place as
        32-bit words, and done, to be called after the device entry point, is the stream handshake's second half.
        Arrays or sequences: checked and converted by pair_arrays, for the host entry point; done is None."""
        if not is_torch(columns):
            c, v = _lib.pair_arrays(columns, values)
            return (None, c.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                    v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), c.size)
        import torch
        if not is_torch(values):
            raise ValueError(f"{what}: columns and values must both be tensors or both arrays")
        if columns.numel() != values.numel():
            raise _lib.IllegalArgumentException("columns and values differ in length")
        if values.dtype == torch.int64 and values.numel() and bool(((values < 0) | (values >= 1 << 31)).any()):
            raise _lib.IllegalArgumentException("Values should be non-negative and below 2^31")
        c = self._words(what, columns)
        v = self._words(what, values)
        done = self._handshake(columns.device)
        done.words = (c, v)  # referenced for as long as the caller holds done
        return done, _dptr(c), _dptr(v), c.numel()

    def from_values(self, values, run_optimize=False) -> int:
        """A resident bitmap from its values, built on the device (rbg_ctx_from_values): RoaringBitmap.bitmapOf
        / add(int...), with run_optimize followed by runOptimize() -> batch id of a one-bitmap batch, the same
        as load([RoaringBitmap.from_values(values, run_optimize)]).  The values need not be sorted or distinct.
        A numpy array or sequence of values below 2^32 is uploaded; a torch tensor on this engine's GPU is read
        in place (rbg_ctx_from_values_device), int64 (the low 32 bits of every element are read, so -1 is
        0xFFFFFFFF) or uint32, with point_query's stream handshake.  Synchronous either way: the container
        count and the batch totals are read back."""
        out = ctypes.c_int32()
        if is_torch(values):
            v = self._words("from_values", values, ("int64", "uint32"))
            done = self._handshake(values.device)
            check(lib().rbg_ctx_from_values_device(self._ctx, _dptr(v), v.numel(), int(bool(run_optimize)),
                                                   ctypes.byref(out)))
            done()
            return out.value
        v = as_u32(values)
        check(lib().rbg_ctx_from_values(self._ctx, v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), v.size,
                                        int(bool(run_optimize)), ctypes.byref(out)))
        return out.value

    def mutate_values(self, batch, values, remove=False):
        """A batch of values added to (remove=False: RoaringBitmap.add(int...) / addN, RB/RoaringBitmap.java
        :483-570) or removed from (remove=True: remove(int) value by value, :2637-2648) a resident bitmap, on the
        device (rbg_ctx_mutate_values) -> (batch id, changed): a new one-bitmap batch, the same as load of the
        reference's bitmap after the calls (a run container stays a run container, an emptied one is dropped, an
        untouched one keeps its bytes), and the number of values actually added or removed (the checkedAdd /
        checkedRemove hits).  The operand stays as it is.  Only the keys the values touch are expanded.  Values
        as from_values takes them: a numpy array or sequence below 2^32 is uploaded; a torch int64 (low 32 bits)
        or uint32 tensor on this engine's GPU is read in place (rbg_ctx_mutate_values_device) with point_query's
        stream handshake.  Synchronous either way."""
        out = ctypes.c_int32()
        changed = ctypes.c_uint64()
        op = _lib.RBG_MUT_REMOVE if remove else _lib.RBG_MUT_ADD
        if is_torch(values):
            v = self._words("mutate_values", values, ("int64", "uint32"))
            done = self._handshake(values.device)
            check(lib().rbg_ctx_mutate_values_device(self._ctx, int(batch), op, _dptr(v), v.numel(), ctypes.byref(out),
                                                     ctypes.byref(changed)))
            done()
            return out.value, int(changed.value)
        v = as_u32(values)
        check(lib().rbg_ctx_mutate_values(self._ctx, int(batch), op, v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                          v.size, ctypes.byref(out), ctypes.byref(changed)))
        return out.value, int(changed.value)

    def add_values(self, batch, values):
        """mutate_values(batch, values, remove=False)"""
        return self.mutate_values(batch, values, False)

    def remove_values(self, batch, values):
        """mutate_values(batch, values, remove=True)"""
        return self.mutate_values(batch, values, True)

    def to_values(self, batch, ia=0, first=0, count=None, dtype=None):
        """The values of ranks [first, first + count) of a resident bitmap (count None: to the end), ascending
        and unsigned: toArray() and the window BatchIterator.nextBatch / limit walk (rbg_ctx_to_values).
        dtype None or numpy's uint32 -> numpy uint32 array, synchronous.  dtype torch.uint32 or torch.int64
        -> a torch tensor on this engine's GPU, written through the device entry point on the engine stream
        with no host synchronisation (but for the first use of a batch, which builds its rank directory);
        torch's current stream waits for it, as with point_query's result."""
        first = int(first)
        count = (1 << 64) - 1 if count is None else int(count)
        if first < 0 or count < 0:
            raise ValueError("to_values: first and count must not be negative")
        n_out = ctypes.c_uint64()
        # the window's size first (a null buffer: no device work): count may reach past the cardinality
        check(lib().rbg_ctx_to_values_device(self._ctx, int(batch), int(ia), first, count, 0, None,
                                             ctypes.byref(n_out)))
        n = int(n_out.value)
        if dtype is not None and is_torch(dtype):
            import torch
            if dtype not in (torch.uint32, torch.int64):
                raise ValueError("to_values: dtype torch.uint32 or torch.int64")
            dev = torch.device("cuda", self.device)
            out = torch.empty(n, dtype=dtype, device=dev)
            if n == 0:
                return out
            done = self._handshake(dev)
            check(lib().rbg_ctx_to_values_device(self._ctx, int(batch), int(ia), first, n,
                                                 int(dtype == torch.int64), ctypes.c_void_p(out.data_ptr()),
                                                 ctypes.byref(n_out)))
            done()
            return out
        if dtype is not None and np.dtype(dtype) != np.uint32:
            raise ValueError("to_values: a numpy result is uint32")
        out = np.empty(n, dtype=np.uint32)
        if n:
            check(lib().rbg_ctx_to_values(self._ctx, int(batch), int(ia), first, n,
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(n_out)))
        return out

    # ---- dense bitsets and masks (bitset.hip): BitSetUtil, RB/BitSetUtil.java ----
    def _from_bitset(self, what, x, layout, torch_dtypes, numpy_dtypes, run_optimize):
        """the shared front of from_words / from_mask: a torch tensor on this engine's GPU is read in place
        (made contiguous, and for packed bytes 8-byte aligned, on the current stream first), anything else
        is uploaded"""
        out = ctypes.c_int32()
        if is_torch(x):
            import torch
            if x.device.type != "cuda" or x.device.index != self.device:
                raise ValueError(f"{what}: the tensor must be on device {self.device}")
            if x.dtype not in [getattr(torch, d) for d in torch_dtypes]:
                raise ValueError(f"{what}: a tensor of {' or '.join(torch_dtypes)} is required")
            t = x.contiguous().reshape(-1)
            if layout == _lib.RBG_BITS_PACKED and t.numel() and t.data_ptr() % 8:
                t = t.clone()  # a byte view at an odd address: a fresh allocation is aligned
            done = self._handshake(x.device)
            check(lib().rbg_ctx_from_bitset_device(self._ctx, _dptr(t), t.numel() * t.element_size()
                                                   if layout == _lib.RBG_BITS_PACKED else t.numel(), layout,
                                                   int(bool(run_optimize)), ctypes.byref(out)))
            done()
            return out.value
        if isinstance(x, (bytes, bytearray, memoryview)):
            v = np.frombuffer(x, dtype=np.uint8)
        else:
            v = np.ascontiguousarray(x)
        if v.dtype not in [np.dtype(d) for d in numpy_dtypes]:
            raise ValueError(f"{what}: an array of {' or '.join(numpy_dtypes)} is required")
        v = v.reshape(-1)
        n = v.nbytes if layout == _lib.RBG_BITS_PACKED else v.size
        check(lib().rbg_ctx_from_bitset(self._ctx, ctypes.c_void_p(v.ctypes.data) if n else None, n, layout,
                                        int(bool(run_optimize)), ctypes.byref(out)))
        return out.value

    def from_words(self, words, run_optimize=False) -> int:
        """A resident bitmap from a dense bitset given as packed little-endian 64-bit words, built on the device
        (rbg_ctx_from_bitset): BitSetUtil.bitmapOf(long[]) (RB/BitSetUtil.java:160-174) and
        bitmapOf(ByteBuffer) (:185-259), with run_optimize followed by runOptimize() -> batch id of a
        one-bitmap batch, the same as from_values of the set bit positions.  A numpy uint64 / int64 array, or
        bytes of any length (a tail of 1..7 bytes is a last word), is uploaded.  A torch int64 / uint8 tensor
        on this engine's GPU is read in place (rbg_ctx_from_bitset_device) with point_query's stream
        handshake: the words are not copied (a non-contiguous tensor, or a uint8 view at an address that is
        not 8-byte aligned, is first made a contiguous aligned one on the current stream), nothing at or past
        the end is read, and three kernels read them, so they must not change until the call returns.  At
        most 2^26 words (2^32 bits): more raises IllegalArgumentException before any device work.
        Synchronous: the container count and the batch totals are read back.  Against torch.nonzero +
        from_values the call was 2 to 23 times faster at every shape measured, 2^24 to 2^32 bits at densities 2^-10
        to 1/2; sparser bitsets were not measured."""
        return self._from_bitset("from_words", words, _lib.RBG_BITS_PACKED, ("int64", "uint8"),
                                 ("uint64", "int64", "uint8"), run_optimize)

    def from_mask(self, mask, run_optimize=False) -> int:
        """The same from a mask, one element per bit position, nonzero = set (so 2 and 255 count): a numpy
        bool / uint8 array, or a torch bool / uint8 tensor on this engine's GPU such as `x > 0`, which one
        kernel packs into pooled words (a non-contiguous mask is made contiguous on the current stream first).
        A mask of n elements sets no bit at or above n.  At most 2^32 elements."""
        return self._from_bitset("from_mask", mask, _lib.RBG_BITS_BYTES, ("bool", "uint8"), ("bool", "uint8"),
                                 run_optimize)

    def _last(self, batch, ia):
        """the largest value of a resident bitmap, -1 for an empty one (the existing previousValue query)"""
        return int(self.point_query("prev", batch, [0xFFFFFFFF], ia)[0])

    def _to_bitset(self, batch, ia, first, n, layout, count, dtype, torch_dtype, numpy_dtype):
        """the shared back of to_words / to_mask: `count` output elements for the window [first, first + n)"""
        if dtype is not None and is_torch(dtype):
            import torch
            if dtype != getattr(torch, torch_dtype):
                raise ValueError(f"a torch result is torch.{torch_dtype}")
            dev = torch.device("cuda", self.device)
            out = torch.empty(count, dtype=dtype, device=dev)
            done = self._handshake(dev) if count else None
            check(lib().rbg_ctx_to_bitset_device(self._ctx, int(batch), int(ia), first, n, layout, _dptr(out)))
            if done:
                done()
            return out
        if dtype is not None and np.dtype(dtype) != np.dtype(numpy_dtype):
            raise ValueError(f"a numpy result is {numpy_dtype}")
        out = np.empty(count, dtype=numpy_dtype)
        check(lib().rbg_ctx_to_bitset(self._ctx, int(batch), int(ia), first, n, layout,
                                      ctypes.c_void_p(out.ctypes.data) if count else None))
        return out

    def to_words(self, batch, ia=0, first_word=0, n_words=None, dtype=None):
        """Words [first_word, first_word + n_words) of a resident bitmap as a dense bitset of little-endian
        64-bit words, expanded on the device (rbg_ctx_to_bitset): BitSetUtil.toLongArray
        (RB/BitSetUtil.java:67-108).  n_words None: toLongArray's own length from the bitmap's last value
        (:76-79: none for an empty bitmap, last / 64 + 1 words for last >= 64, 2 words for every last in
        0..63), and IllegalArgumentException("bitmap has negative bits set") for a last value of at least
        2^31 (:72-75); an explicit window may cover the whole 32-bit universe (2^26 words).  Absent keys and
        everything past the last value are zero words.  dtype None -> numpy uint64, synchronous; torch.int64
        -> a tensor on this engine's GPU written on the engine stream with no host synchronisation (the
        current stream waits for it, as with to_values).  Every word of the window is written once: the
        output is not zeroed first."""
        first_word = int(first_word)
        if n_words is None:
            last = self._last(batch, ia)
            if last >= 1 << 31:
                raise _lib.IllegalArgumentException("bitmap has negative bits set")
            n_words = max((max(last, 64) // 64 + 1 if last >= 0 else 0) - first_word, 0)
        n_words = int(n_words)
        if first_word < 0 or n_words < 0:
            raise ValueError("to_words: first_word and n_words must not be negative")
        return self._to_bitset(batch, ia, 64 * first_word, 64 * n_words, _lib.RBG_BITS_PACKED, n_words, dtype,
                               "int64", "uint64")

    def to_mask(self, batch, ia=0, first=0, n=None, dtype=None):
        """Bit positions [first, first + n) of a resident bitmap as a mask, one element each (any first; n
        None: up to the last value, nothing for an empty bitmap): dtype None -> numpy bool, synchronous;
        torch.bool -> a tensor on this engine's GPU, as to_words gives one.  Against to_values + an indexed
        store into a zeroed mask the call was 1.8 to 8.6 times faster at every shape measured."""
        first = int(first)
        if n is None:
            n = max(self._last(batch, ia) + 1 - first, 0)
        n = int(n)
        if first < 0 or n < 0:
            raise ValueError("to_mask: first and n must not be negative")
        return self._to_bitset(batch, ia, first, n, _lib.RBG_BITS_BYTES, n, dtype, "bool", "bool")

    def bsi_from_columns(self, columns, values, run_optimize=False):
        """A resident bit-sliced index from (column, value) pairs, built on the device
        (rbg_ctx_bsi_from_columns): setValue(column, value) for every pair, with run_optimize followed by
        runOptimize() -> (batch, nbits, minValue, maxValue), the batch being the key-major [ebM, bA[0..nbits-1]]
        that load([ebM] + slices) of RoaringBitmapSliceIndex.from_columns gives, as bsi / bsi_buffer take it.
        The pairs may come in any order; a negative value or a repeated column raises
        IllegalArgumentException, as do columns and values of different lengths.  numpy arrays or sequences
        (columns below 2^32, values below 2^31) are uploaded; torch tensors on this engine's GPU are read
        in place (rbg_ctx_bsi_from_columns_device), int64 (the low 32 bits of every element are read) or
        uint32 / int32, with point_query's stream handshake.  Synchronous either way."""
        done, cp, vp, n = self._pairs("bsi_from_columns", columns, values)
        f = lib().rbg_ctx_bsi_from_columns_device if done else lib().rbg_ctx_bsi_from_columns
        got = _index_call(f, self._ctx, cp, vp, n, int(bool(run_optimize)))
        if done:
            done()
        return got

    def bsi_add(self, a, nbits_a, b, nbits_b, min_a=0, max_a=0):
        """RoaringBitmapSliceIndex.add (BSI/:66-95) of two resident run-free indexes, the key-major batches
        [ebM, bA[0..nbits_a-1]] and [ebM, bA[0..nbits_b-1]], fused on the device (rbg_ctx_bsi_add)
        -> (batch, nbits, minValue, maxValue): a new batch, the one load() of the reference's result bitmaps
        gives, as bsi / bsi_buffer / bsi_get_values / bsi_to_pairs take it.  Both operands stay; a == b
        doubles the values.  An empty ebM of b: a copy of a with (nbits_a, min_a, max_a).  A run container
        in either batch, more than 32 slices on either side or in the sum: IllegalArgumentException, no
        batch made.  Synchronous."""
        return _index_call(lib().rbg_ctx_bsi_add, self._ctx, int(a), int(nbits_a), int(b), int(nbits_b), int(min_a),
                           int(max_a))

    def bsi_set_values(self, batch, nbits, columns, values, min_value=0, max_value=0):
        """RoaringBitmapSliceIndex.setValues(List<Pair>) (BSI/:349-357; setValue, :299-313, with one pair) on a
        resident index, the key-major batch [ebM, bA[0..nbits-1]] with the fields min_value / max_value, on the
        device (rbg_ctx_bsi_set_values) -> (batch, nbits, minValue, maxValue): a new batch, the one load() of
        the reference's bitmaps after the call gives, as bsi / bsi_buffer / bsi_get_values / bsi_to_pairs /
        bsi_add take it.  The operand stays.  The pairs apply in order: a column given many times keeps its last
        value.  nbits / minValue / maxValue follow ensureCapacityInternal (BSI/:315-326): they are the
        reference's fields, not the true extremes, and only bits below the new nbits are kept.  A negative
        value, no pair at all, a batch of another shape, a run container in a slice or one in ebM that is not
        full: IllegalArgumentException, no batch made.  numpy arrays or sequences are uploaded; torch tensors
        on this engine's GPU are read in place (rbg_ctx_bsi_set_values_device), as in bsi_from_columns.
        Synchronous either way."""
        done, cp, vp, n = self._pairs("bsi_set_values", columns, values)
        f = lib().rbg_ctx_bsi_set_values_device if done else lib().rbg_ctx_bsi_set_values
        got = _index_call(f, self._ctx, int(batch), int(nbits), int(min_value), int(max_value), cp, vp, n)
        if done:
            done()
        return got

    def bsi_in(self, batch, nbits, values, parallelism=1, has_found=False) -> int:
        """BitSliceIndexBase.parallelIn (BBSI/:611-639), WHERE value IN (values), over a resident index
        [ebM, bA[0..nbits-1], foundSet?] in one fused device pass (rbg_ctx_bsi_in) -> batch id of a new
        one-bitmap batch: the columns of ebM (and of the foundSet) whose value is in the list, as the batch
        load() of the reference's result gives -- usable in pairwise, to_values and batch_fetch.  values: any
        iterable of ints that fit 32 bits (a negative entry is its bit pattern: it matches only with 32
        slices), in any order, repeats allowed.  parallelism only decides whether a full container is a
        bitmap or a run container.  parallelism < 1, nbits > 32 or a batch of another shape:
        IllegalArgumentException, no batch made.  Synchronous."""
        v = _lib.in_list(values)
        out = ctypes.c_int32()
        check(lib().rbg_ctx_bsi_in(self._ctx, int(batch), int(nbits), int(bool(has_found)),
                                   v.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), v.size, int(parallelism),
                                   ctypes.byref(out)))
        return out.value

    def bsi_transpose(self, batch, nbits, parallelism=1, has_found=False):
        """BitSliceIndexBase.parallelTransposeWithCount (BBSI/:551-597), GROUP BY value / COUNT(*), over a
        resident index [ebM, bA[0..nbits-1], foundSet?] on the device (rbg_ctx_bsi_transpose)
        -> (batch, nbits, minValue, maxValue): a new key-major batch [ebM, bA[0..nbits-1]] whose columns are
        the distinct 32-bit values of the columns of ebM (and of the foundSet) and whose values are how many
        columns held each -- the batch load() of the reference's result bitmaps gives, as bsi / bsi_buffer /
        bsi_get_values / bsi_to_pairs / bsi_add / bsi_in take it.  nbits is the bit count of the largest
        count, min / max the smallest and largest count; no column: one empty bitmap and (0, 0, 0).
        parallelism only decides whether a full container of the result's ebM is a bitmap or a run container.
        parallelism < 1, nbits > 32 or a batch of another shape: IllegalArgumentException, no batch made.
        Synchronous."""
        return _index_call(lib().rbg_ctx_bsi_transpose, self._ctx, int(batch), int(nbits), int(bool(has_found)),
                           int(parallelism))

    def bsi_get_values(self, batch, nbits, columns, has_found=False):
        """getValue for many columns at once against a resident index [ebM, bA[0..nbits-1], foundSet?]
        (rbg_ctx_bsi_get_values): one int64 per column, in query order, -1 where ebM lacks the column.  The
        columns need not be sorted or distinct.  numpy in -> numpy out, synchronous; a torch tensor on this
        engine's GPU (int64 low words, or uint32) -> torch int64 tensor through the device entry point with no
        host synchronisation, under point_query's stream handshake."""
        if is_torch(columns):
            import torch
            q = self._words("bsi_get_values", columns)
            out = torch.empty(q.numel(), dtype=torch.int64, device=columns.device)
            if q.numel() == 0:
                return out
            done = self._handshake(columns.device)
            check(lib().rbg_ctx_bsi_get_values_device(self._ctx, int(batch), int(nbits), int(bool(has_found)),
                                                      ctypes.c_void_p(q.data_ptr()), q.numel(),
                                                      ctypes.c_void_p(out.data_ptr())))
            done()
            return out
        q = as_u32(columns)
        out = np.empty(q.size, dtype=np.int64)
        check(lib().rbg_ctx_bsi_get_values(self._ctx, int(batch), int(nbits), int(bool(has_found)),
                                           q.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), q.size,
                                           out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
        return out

    def bsi_pairs_count(self, batch, nbits, has_found=False) -> int:
        """The pairs bsi_to_pairs would write (cardinality of ebM): a null-output call, no device work."""
        n_out = ctypes.c_uint64()
        check(lib().rbg_ctx_bsi_to_pairs_device(self._ctx, int(batch), int(nbits), int(bool(has_found)), 0, 0, None,
                                                None, ctypes.byref(n_out)))
        return int(n_out.value)

    def bsi_to_pairs(self, batch, nbits, dtype=None, has_found=False):
        """toPairList() of a resident index (rbg_ctx_bsi_to_pairs): every column of ebM, ascending and
        unsigned, with its value -> (columns, values).  dtype None: numpy uint32 columns and int32 values,
        synchronous.  dtype torch.uint32 or torch.int64: torch tensors on this engine's GPU (columns of
        that dtype; values int32 with uint32 columns, int64 with int64 columns), written through the device
        entry point on the engine stream with no host synchronisation; torch's current stream waits for
        them, as with point_query's result."""
        n = self.bsi_pairs_count(batch, nbits, has_found)
        n_out = ctypes.c_uint64()
        if dtype is not None and is_torch(dtype):
            import torch
            if dtype not in (torch.uint32, torch.int64):
                raise ValueError("bsi_to_pairs: dtype torch.uint32 or torch.int64")
            wide = int(dtype == torch.int64)
            dev = torch.device("cuda", self.device)
            cols = torch.empty(n, dtype=dtype, device=dev)
            vals = torch.empty(n, dtype=torch.int64 if wide else torch.int32, device=dev)
            if n == 0:
                return cols, vals
            done = self._handshake(dev)
            check(lib().rbg_ctx_bsi_to_pairs_device(self._ctx, int(batch), int(nbits), int(bool(has_found)), wide, wide,
                                                    ctypes.c_void_p(cols.data_ptr()), ctypes.c_void_p(vals.data_ptr()),
                                                    ctypes.byref(n_out)))
            done()
            return cols, vals
        if dtype is not None and np.dtype(dtype) != np.uint32:
            raise ValueError("bsi_to_pairs: numpy columns are uint32")
        cols = np.empty(n, dtype=np.uint32)
        vals = np.empty(n, dtype=np.int32)
        if n:
            check(lib().rbg_ctx_bsi_to_pairs(self._ctx, int(batch), int(nbits), int(bool(has_found)), 0, 0,
                                             cols.ctypes.data_as(ctypes.c_void_p), vals.ctypes.data_as(ctypes.c_void_p),
                                             ctypes.byref(n_out)))
        return cols, vals

    # ---- the range-encoded index (RangeBitmap, rbg_ctx_rangebitmap_*) -----------
    def rangebitmap_load(self, index) -> int:
        """RangeBitmap.map of a serialized index (bytes, or a RangeBitmap), kept resident -> index handle (not
        a batch id)."""
        b = index.serialize() if hasattr(index, "serialize") else bytes(index)
        out = ctypes.c_int32()
        check(lib().rbg_ctx_rangebitmap_load(self._ctx, b, len(b), ctypes.byref(out)))
        return out.value

    def rangebitmap_build(self, values, maxValue=None) -> int:
        """RangeBitmap.appender(maxValue), add for every value in order, build -- on the device
        (rbg_ctx_rangebitmap_build) -> index handle, the one rangebitmap_load gives for the Appender's stream
        of the same values.  A numpy uint64 / int64 array (int64 taken as its bit pattern, as add_many takes
        it) is uploaded.  A torch int64 tensor on this engine's GPU is read in place
        (rbg_ctx_rangebitmap_build_device) with point_query's stream handshake: the values are not copied (a
        non-contiguous tensor is first made contiguous on the current stream) and must not change until the
        call returns.  maxValue=None: the largest value given.  A value outside maxValue's mask raises
        IllegalArgumentException("... too large") and builds nothing (the reference's add throws at that row).
        Synchronous: the largest value and the arena's size are read back."""
        out = ctypes.c_int32()
        from_data = maxValue is None
        mx = 0 if from_data else int(maxValue) & 0xFFFFFFFFFFFFFFFF
        if is_torch(values):
            import torch
            if values.device.type != "cuda" or values.device.index != self.device:
                raise ValueError(f"rangebitmap_build: the tensor must be on device {self.device}")
            if values.dtype != torch.int64:
                raise ValueError("rangebitmap_build: a tensor of int64 is required")
            t = values.contiguous().reshape(-1)
            done = self._handshake(values.device)
            check(lib().rbg_ctx_rangebitmap_build_device(self._ctx, _dptr(t), t.numel(), mx, int(from_data),
                                                         ctypes.byref(out)))
            done()
            return out.value
        v = np.asarray(values)
        if v.dtype not in (np.dtype(np.uint64), np.dtype(np.int64)):
            raise ValueError("rangebitmap_build: an array of uint64 or int64 is required")
        v = np.ascontiguousarray(v).reshape(-1)
        check(lib().rbg_ctx_rangebitmap_build(self._ctx, ctypes.c_void_p(v.ctypes.data) if v.size else None, v.size,
                                              mx, int(from_data), ctypes.byref(out)))
        return out.value

    def rangebitmap_serialize(self, index) -> bytes:
        """Appender.serialize of a resident index, loaded or built (rbg_ctx_rangebitmap_serialize): for a built
        one the Appender's bytes, for a loaded one the bytes that were mapped."""
        return call_bytes(lib().rbg_ctx_rangebitmap_serialize, self._ctx, int(index))

    def rangebitmap_release(self, index):
        check(lib().rbg_ctx_rangebitmap_release(self._ctx, int(index)))

    def rangebitmap_info(self, index) -> dict:
        s = (ctypes.c_uint64 * 6)()
        check(lib().rbg_ctx_rangebitmap_info(self._ctx, int(index), s))
        return dict(zip(["slices", "blocks", "rows", "mask", "payload_bytes"], [int(x) for x in s]))

    def rangebitmap_query(self, index, op, a, b=0, context=None, context_i=0) -> int:
        """lte / lt / gt / gte / eq / neq (a) or between (a, b) of a resident index, optionally intersected
        with bitmap context_i of the batch `context` -> a new one-bitmap batch, as pairwise's operands are."""
        out = ctypes.c_int32()
        check(lib().rbg_ctx_rangebitmap_query(self._ctx, int(index), _lib.RANGEBITMAP_OP.get(op, op),
                                              int(a) & 0xFFFFFFFFFFFFFFFF, int(b) & 0xFFFFFFFFFFFFFFFF,
                                              -1 if context is None else int(context), int(context_i),
                                              ctypes.byref(out)))
        return out.value

    def rangebitmap_count(self, index, op, a, b=0, context=None, context_i=0) -> int:
        """the *Cardinality form of rangebitmap_query, reduced on the device (synchronous)"""
        out = ctypes.c_int64()
        check(lib().rbg_ctx_rangebitmap_count(self._ctx, int(index), _lib.RANGEBITMAP_OP.get(op, op),
                                              int(a) & 0xFFFFFFFFFFFFFFFF, int(b) & 0xFFFFFFFFFFFFFFFF,
                                              -1 if context is None else int(context), int(context_i),
                                              ctypes.byref(out)))
        return out.value

    def batch_counts(self, batch) -> np.ndarray:
        """containers per input bitmap of a batch"""
        n = self.batch_stats(batch)["bitmaps"]
        out = np.zeros(n, dtype=np.uint32)
        check(lib().rbg_ctx_batch_counts(self._ctx, int(batch), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                         n))
        return out

    def wide_card(self, op, batch, key_lo=0, key_hi=65536):
        check(lib().rbg_ctx_wide_card(self._ctx, _lib.WIDE_CARD_OP[op], int(batch), int(key_lo), int(key_hi)))

    def batch_and_card(self, batch):
        check(lib().rbg_ctx_batch_and_card(self._ctx, int(batch)))

    # ---- results (synchronous) -------------------------------------------------
    def card(self) -> int:
        out = ctypes.c_int32()
        check(lib().rbg_ctx_card(self._ctx, ctypes.byref(out)))
        return out.value

    def cards(self, n) -> np.ndarray:
        out = np.zeros(n, dtype=np.int32)
        check(lib().rbg_ctx_cards(self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), n))
        return out

    def result_stats(self) -> dict:
        s = (ctypes.c_int64 * 4)()
        check(lib().rbg_ctx_result_stats(self._ctx, s))
        return {"containers": s[0], "payload_bytes": s[1], "has_run": s[2], "cardinality": s[3]}

    def serialize(self):
        """Enqueue the on-device portable serialization of the last result."""
        check(lib().rbg_ctx_serialize(self._ctx))

    def fetch(self) -> RoaringBitmap:
        return RoaringBitmap(call_bytes(lib().rbg_ctx_fetch, self._ctx))

    def fetch_shard_device(self, total_containers, has_run, payload_base, desc, offsets, runflags, payload):
        """Enqueue the pending result as a key shard of a global bitmap, written straight into
        device memory (torch tensors or raw pointers; offsets / runflags may be None when the
        global layout has no offset table / no run container).  Asynchronous: sync() before use."""
        def ptr(t):
            if t is None:
                return None
            return int(t) if isinstance(t, int) else int(t.data_ptr())
        check(lib().rbg_ctx_fetch_shard_device(self._ctx, int(total_containers), int(bool(has_run)), int(payload_base),
                                               ptr(desc), ptr(offsets), ptr(runflags), ptr(payload)))

    def result_layout_device(self, dst3):
        """Enqueue (containers, payload bytes, has_run) of the pending result into a device int64
        tensor of 3 elements on the engine stream (the input of a device all-gather)."""
        check(lib().rbg_ctx_result_layout_device(self._ctx, ctypes.c_void_p(dst3.data_ptr())))

    def fetch_shard_device_dyn(self, layout, rank, world, out, runb=None):
        """Enqueue this rank's slice of the global bitmap, placed by a device-resident layout
        (world x 3 int64 tensor, key-range order), into `out` (a uint8 tensor laid out as the whole
        global bitmap) and one run byte per global container into runb.  No host synchronisation."""
        check(lib().rbg_ctx_fetch_shard_device_dyn(self._ctx, ctypes.c_void_p(layout.data_ptr()), int(rank),
                                                   int(world), ctypes.c_void_p(out.data_ptr()),
                                                   ctypes.c_void_p(runb.data_ptr()) if runb is not None else None))

    def fetch_shard(self, total_containers, has_run, first_container, payload_base):
        d, o, p = _lib.rbg_buffer(), _lib.rbg_buffer(), _lib.rbg_buffer()
        check(lib().rbg_ctx_fetch_shard(self._ctx, int(total_containers), int(has_run), int(first_container),
                                        int(payload_base), ctypes.byref(d), ctypes.byref(o), ctypes.byref(p)))
        return take(d), take(o), take(p)
