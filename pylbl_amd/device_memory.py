"""Memory the engine hands out: spectra left in HBM (DeviceSpectra), and the pools that recycle
HBM blocks (DevicePool) and page-locked host arrays (PinnedPool) for one Engine."""
from ctypes import byref, c_void_p
import threading
import weakref

import numpy as np

from .abi import ASYNC, LBL_OK


class DeviceSpectra(object):
    """Spectra left in HBM: [levels, n] float64 on the engine's GPU."""
    def __init__(self, engine, levels, n):
        self.engine = engine
        self.shape = (int(levels), int(n))
        self.pointer = c_void_p()
        engine._check(engine.lib.lbl_device_alloc(engine.handle, self.shape[0]*self.shape[1]*8,
                                                  byref(self.pointer)))

    def to_host(self):
        out = np.empty(self.shape, dtype=np.float64)
        self.engine._check(self.engine.lib.lbl_copy_to_host(
            self.engine.handle, out.ctypes.data, self.pointer, out.nbytes))
        return out

    def to_host_into(self, target, columns=None, asynchronous=False):
        """Copies the first `columns` values of every row straight into `target`, a float64
        array view [rows, columns] whose rows are contiguous (any row stride), e.g.
        beta[:, mechanism, :].  asynchronous: queue the copy behind everything queued so far
        and return; Engine.synchronize() waits for it (use page-locked targets,
        Engine.host_array, or the copy blocks anyway)."""
        columns = self.shape[1] if columns is None else int(columns)
        if target.dtype != np.float64 or target.shape != (self.shape[0], columns) or \
                columns > self.shape[1] or (columns > 1 and target.strides[1] != 8) or \
                (self.shape[0] > 1 and target.strides[0] < columns*8):
            raise ValueError("target must be float64[rows, columns] with contiguous rows.")
        pitch = target.strides[0] if self.shape[0] > 1 else columns*8
        self.engine._check(self.engine.lib.lbl_copy_rows_to_host(
            self.engine.handle, target.ctypes.data, pitch, self.pointer, self.shape[1]*8,
            columns*8, self.shape[0], ASYNC if asynchronous else 0))
        return target

    def rows(self, count):
        """The first `count` rows of this block, as a DeviceSpectra that owns no memory (valid
        while this block is)."""
        if not 0 < int(count) <= self.shape[0]:
            raise ValueError(f"rows({count}) of a block of {self.shape[0]} rows.")
        return _DeviceRows(self, int(count))

    def free(self):
        if self.pointer:
            self.engine.lib.lbl_device_free(self.engine.handle, self.pointer)
            self.pointer = c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class _DeviceRows(DeviceSpectra):
    """DeviceSpectra.rows: leading rows of a block; freeing it frees nothing."""
    def __init__(self, block, count):
        self.engine = block.engine
        self.block = block
        self.shape = (count, block.shape[1])
        self.pointer = block.pointer

    def free(self):
        pass


class DevicePool(object):
    """[levels, n] blocks in HBM handed out and taken back (hipMalloc / hipFree cost more than
    the continuum kernels that fill such a block, and hipFree stops the device)."""
    def __init__(self, engine, limit=32 << 30):
        self.engine = weakref.ref(engine)
        self.limit = limit
        self.idle = {}          # shape -> [DeviceSpectra]
        self.idle_bytes = 0
        self.lock = threading.RLock()       # blocks are taken and given by any thread

    def take(self, levels, n):
        shape = (int(levels), int(n))
        with self.lock:
            blocks = self.idle.get(shape)
            if blocks:
                self.idle_bytes -= shape[0]*shape[1]*8
                return blocks.pop()
        return DeviceSpectra(self.engine(), *shape)

    def give(self, block):
        size = block.shape[0]*block.shape[1]*8
        with self.lock:
            if block.pointer and self.idle_bytes + size <= self.limit:
                self.idle.setdefault(tuple(block.shape), []).append(block)
                self.idle_bytes += size
                return
        block.free()

    def clear(self):
        with self.lock:
            idle, self.idle, self.idle_bytes = self.idle, {}, 0
        for blocks in idle.values():
            for block in blocks:
                block.free()


class PinnedPool(object):
    """Page-locked host arrays for results.  Pinning memory is slow, so buffers are recycled:
    when the last view of an array handed out here is garbage-collected its buffer goes back
    to the pool (up to `limit` bytes of idle buffers are kept)."""
    def __init__(self, engine, limit=8 << 30):
        self.engine = weakref.ref(engine)
        self.limit = limit
        self.idle = []          # (capacity, pointer)
        self.idle_bytes = 0
        # Arrays are handed out to any thread and come back from whichever thread drops the last
        # view (a finalizer: it may run inside array() on the same thread, hence re-entrant).
        self.lock = threading.RLock()

    def array(self, shape):
        shape = tuple(int(x) for x in shape)
        count = int(np.prod(shape)) if shape else 1
        nbytes = max(count*8, 8)
        engine = self.engine()
        with self.lock:
            best = None
            for i, (capacity, _) in enumerate(self.idle):
                if nbytes <= capacity <= 2*nbytes + (1 << 20) and \
                        (best is None or capacity < self.idle[best][0]):
                    best = i
            if best is not None:
                capacity, pointer = self.idle.pop(best)
                self.idle_bytes -= capacity
        if best is None:
            capacity, handle = nbytes, c_void_p()
            if engine.lib.lbl_host_alloc(engine.handle, capacity, byref(handle)) != LBL_OK:
                # No more page-locked memory to be had (results held by the caller count):
                # ordinary memory still works, copies into it are only slower.
                self.clear()
                return np.empty(shape, dtype=np.float64)
            pointer = handle.value
        from ctypes import c_char
        buffer = (c_char*capacity).from_address(pointer)
        weakref.finalize(buffer, PinnedPool._release, weakref.ref(self), capacity, pointer)
        return np.frombuffer(buffer, dtype=np.float64, count=count).reshape(shape)

    @staticmethod
    def _release(pool, capacity, pointer):
        pool = pool()
        engine = pool.engine() if pool is not None else None
        if engine is None or not engine.handle:
            return                      # engine gone: the runtime reclaims the pages at exit
        with pool.lock:
            if pool.idle_bytes + capacity <= pool.limit:
                pool.idle.append((capacity, pointer))
                pool.idle_bytes += capacity
                return
        engine.lib.lbl_host_free(engine.handle, c_void_p(pointer))

    def clear(self):
        engine = self.engine()
        with self.lock:
            idle, self.idle, self.idle_bytes = self.idle, [], 0
        for _, pointer in idle:
            if engine is not None and engine.handle:
                engine.lib.lbl_host_free(engine.handle, c_void_p(pointer))
