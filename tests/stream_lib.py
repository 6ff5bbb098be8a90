"""ctypes access to tests/native/libstream_probe.so - the CALLER's side of a HIP stream (test infrastructure, built by
build.build_test_native): streams and events of the caller's own, a kernel that keeps a stream busy for a given time, a
device-side copy and fill as the caller's own work, and a host read that is not ordered behind a non-blocking stream.
The library links the HIP runtime the device library is linked with, so a stream made here is one the context can use."""
import contextlib
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "tests", "native", "libstream_probe.so")
KINDS = ("default", "blocking", "nonblocking")
BUSY_MAX_US = 20000

_lib = None


def world_inputs():
    """(database, queries) of tests/test_gpu_caller_stream.py's World, for it and for tests/torch_stream_child.py: 6000
    entries of 4..70 SSEs sorted by size (five order buckets), a 12-SSE and a 40-SSE query (two size classes)"""
    import cuda_satabsearch_amd as sat
    return sat.synth.make_db(6000, 4, 70, seed=21, sort=True), [sat.synth.make_query(12, seed=5), sat.synth.make_query(40, seed=6)]


def lib():
    global _lib
    if _lib is None:
        l = C.CDLL(LIB)
        vp, sz, i32p = C.c_void_p, C.c_size_t, C.c_void_p
        for name, args in (("stream_create", [C.c_int, C.POINTER(vp)]), ("stream_destroy", [vp]), ("stream_sync", [vp]),
                           ("busy", [vp, C.c_int]), ("copy_i32", [vp, i32p, i32p, sz]), ("fill_i32", [vp, i32p, C.c_int32, sz]),
                           ("event_create", [C.POINTER(vp)]), ("event_record", [vp, vp]), ("event_sync", [vp]),
                           ("event_destroy", [vp]), ("alloc_i32", [sz, C.POINTER(vp)]), ("free_i32", [i32p]),
                           ("alloc_bytes", [C.c_void_p, C.POINTER(sz)]),
                           ("read_unordered", [C.c_void_p, i32p, sz])):
            fn = getattr(l, name)
            fn.argtypes, fn.restype = args, C.c_int
        _lib = l
    return _lib


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %d" % (what, rc))


def stream_create(blocking):
    out = C.c_void_p()
    _ok(lib().stream_create(int(bool(blocking)), C.byref(out)), "stream_create")
    return out.value or 0


def stream_destroy(stream):
    _ok(lib().stream_destroy(stream), "stream_destroy")


def stream_sync(stream):
    _ok(lib().stream_sync(stream or None), "stream_sync")


def busy(stream, microseconds):
    """keep `stream` (0: the default stream) busy for that long; never more than 20 ms"""
    assert 1 <= microseconds <= BUSY_MAX_US, microseconds
    _ok(lib().busy(stream or None, int(microseconds)), "busy")


def copy_i32(stream, dst, src, n):
    _ok(lib().copy_i32(stream or None, dst, src, int(n)), "copy_i32")


def fill_i32(stream, dst, value, n):
    _ok(lib().fill_i32(stream or None, dst, int(value), int(n)), "fill_i32")


def event_create():
    out = C.c_void_p()
    _ok(lib().event_create(C.byref(out)), "event_create")
    return out.value


def event_record(event, stream):
    _ok(lib().event_record(event, stream or None), "event_record")


def event_sync(event):
    _ok(lib().event_sync(event), "event_sync")


def event_destroy(event):
    _ok(lib().event_destroy(event), "event_destroy")


def alloc_i32(n):
    out = C.c_void_p()
    _ok(lib().alloc_i32(int(n), C.byref(out)), "alloc_i32")
    return out.value


def free(ptr):
    _ok(lib().free_i32(ptr), "free_i32")


def alloc_bytes(ptr):
    """the size in bytes of the device allocation that holds `ptr` (hipMemGetAddressRange)"""
    out = C.c_size_t(0)
    _ok(lib().alloc_bytes(ptr, C.byref(out)), "alloc_bytes")
    return int(out.value)


def read_unordered(src, n):
    """int32[n] at device address `src` by a plain synchronous copy: ordered behind the default stream and blocking
    streams only"""
    out = np.empty(int(n), np.int32)
    _ok(lib().read_unordered(out.ctypes.data, src, int(n)), "read_unordered")
    return out


def wait_behind(stream):
    """record an event behind everything queued on `stream` so far and wait for it - the caller's way to wait for its
    own stream without asking the context"""
    ev = event_create()
    try:
        event_record(ev, stream)
        event_sync(ev)
    finally:
        event_destroy(ev)


@contextlib.contextmanager
def buffer_i32(n):
    p = alloc_i32(n)
    try:
        yield p
    finally:
        free(p)


@contextlib.contextmanager
def caller_stream(kind):
    """the handle to pass to Searcher.use_stream: 0 for "default", else a stream of the caller's own, destroyed (after
    it has drained) on the way out - a context that used it must have switched away or be closed by then"""
    assert kind in KINDS, kind
    if kind == "default":
        yield 0
        return
    s = stream_create(kind == "blocking")
    try:
        yield s
    finally:
        stream_sync(s)
        stream_destroy(s)
