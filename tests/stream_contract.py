"""A harness that makes work on the wrong stream visible (csrc/dyd_common.h: "`_dev` entry points launch on exactly the
hipStream_t they are given").  One side stream `s` carries a delay; behind the delay it copies the real inputs over decoys and
fills the outputs with their sentinels.  An entry that is called with `s` while the delay runs sees the real inputs and writes
after the fill only if every one of its launches, copies and memsets is ordered on `s`:

  * a kernel or copy that reads an input on another stream runs at once and reads the decoy (a valid table of the same shape
    whose results differ in every output, tests/test_stream_contract_cpu.py);
  * a kernel or memset that writes an output on another stream runs at once and is overwritten by the delayed fill.

Both give a mismatch against the reference of the real table.  The helpers of the test modules take the harness as `hz`;
without one they get PLAIN, which uploads, calls on torch's current stream and synchronises as they always did.

The decoy builders at the end are plain numpy and need no GPU."""
import ctypes as C

import numpy as np

MIN_DELAY_MS = 30.0
_CAL = {}


def _dev():
    import torch

    return torch, torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------- the delay
def _spin(units):
    """the delay on the current stream: torch.cuda._sleep(cycles), or a loop of elementwise passes over a large tensor"""
    torch, dev = _dev()
    if _CAL["sleep"]:
        torch.cuda._sleep(int(units))
    else:
        big = _CAL["big"]
        for _ in range(int(units)):
            big.add_(1.0)


def _timed(s, units):
    torch, _ = _dev()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(s):
        e0.record()
        _spin(units)
        e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate():
    """-> (units, measured ms): the length of the delay, found once per session with two events so that it lasts at least
    MIN_DELAY_MS (the aim is half as much again; what guards a test is the `not s.query()` of fire(), not this number)"""
    if "units" in _CAL:
        return _CAL["units"], _CAL["ms"]
    torch, dev = _dev()
    s = torch.cuda.Stream(dev)
    for use_sleep in (True, False):
        if use_sleep and not hasattr(torch.cuda, "_sleep"):
            continue
        _CAL["sleep"] = use_sleep
        if not use_sleep:
            _CAL["big"] = torch.zeros(1 << 26, dtype=torch.float32, device=dev)
        units = 4_000_000 if use_sleep else 8
        _timed(s, units)                                              # the first launch pays for loading the kernel
        ms = _timed(s, units)
        for _ in range(8):
            if ms >= 1.5 * MIN_DELAY_MS:
                break
            units = int(units * min(max(1.7 * MIN_DELAY_MS / max(ms, 1e-3), 1.5), 64.0)) + 1
            ms = _timed(s, units)
        if ms >= MIN_DELAY_MS:
            _CAL["units"], _CAL["ms"] = units, ms
            print(f"stream_contract: delay = {'torch.cuda._sleep' if use_sleep else 'elementwise passes'}({units}) = {ms:.1f} ms")
            return units, ms
    raise AssertionError("no delay of %g ms could be made on the GPU" % MIN_DELAY_MS)


# ---------------------------------------------------------------------------------------------------------- the side stream
def _runs_beside(busy, elsewhere):
    """does the work of elsewhere() finish while `busy` still holds the delay?  Streams are spread over a few hardware queues
    (four by default), and two streams on one queue run one after the other whatever their flags say: behind such a stream
    stray work would wait for the delay like work on the right stream, and a test would prove nothing."""
    torch, _ = _dev()
    with torch.cuda.stream(busy):
        _spin(_CAL["units"])
    elsewhere()
    beside = not busy.query()
    busy.synchronize()
    return beside


def _on_the_null_stream():
    torch, dev = _dev()
    torch.zeros(16, device=dev).add_(1.0)
    e = torch.cuda.Event()
    e.record()
    e.synchronize()


def _on_the_library_stream():
    """a host-pointer entry stages, launches and waits on the library's own stream"""
    from deal_yolo_daya_amd import _native

    _native.hash128(np.frombuffer(b"abcdefgh", np.uint8), np.asarray([0, 3, 8], np.int64))


def side_stream():
    """the stream every harness arms: one that demonstrably runs beside both streams stray work can land on, the null stream
    and the library's own (measured once per session; the torch pool hands out 32 streams in turn)"""
    if "side" in _CAL:
        return _CAL["side"]
    torch, dev = _dev()
    calibrate()
    _on_the_null_stream()                                             # loaded and initialised before anything is measured
    _on_the_library_stream()
    tried = []
    for _ in range(32):
        s = torch.cuda.Stream(dev)
        tried.append(s)                                               # kept: the pool must move on to its next stream
        if _runs_beside(s, _on_the_null_stream) and _runs_beside(s, _on_the_library_stream):
            _CAL["side"] = s
            print(f"stream_contract: side stream no. {len(tried)} runs beside the null stream and the library's stream")
            return s
    raise AssertionError("no stream runs beside the null stream and the library's stream: wrong-stream work cannot be told apart")


def other_stream(a):
    """a second stream for the interleaving tests: one that runs beside `a` if there is one, else any other"""
    torch, dev = _dev()
    key = ("other", a.cuda_stream)
    if key not in _CAL:
        cands = [s for s in (torch.cuda.Stream(dev) for _ in range(32)) if s.cuda_stream != a.cuda_stream]
        beside_a = None
        for k, s in enumerate(cands):                                 # the first that runs beside all three; else beside `a`; else any
            if _runs_beside(a, lambda: (_in(s), s.synchronize())):
                beside_a = beside_a or s
                if _runs_beside(s, _on_the_null_stream) and _runs_beside(s, _on_the_library_stream):
                    _CAL[key] = s
                    print(f"stream_contract: second stream no. {k + 1} runs beside the first, the null stream and the library's stream")
                    break
        else:
            _CAL[key] = beside_a or cands[0]
            print("stream_contract: second stream: none runs beside all three; one beside the first: %s" % (beside_a is not None))
    return _CAL[key]


def _in(s):
    torch, dev = _dev()
    with torch.cuda.stream(s):
        torch.zeros(16, device=dev).add_(1.0)


# ---------------------------------------------------------------------------------------------------------- harnesses
class Plain:
    """what the helpers did before there was a harness: nothing armed, torch's current stream, a device-wide wait"""
    decoy = None
    armed = False

    def arm(self, tensors, decoys=None):
        pass

    def watch(self, *tensors):
        pass

    def call(self, fn, *args):
        torch, _ = _dev()
        return fn(*args, torch.cuda.current_stream().cuda_stream)

    def restore(self):
        torch, _ = _dev()
        torch.cuda.synchronize()


PLAIN = Plain()


def _bytes(t):
    """a flat byte view of a contiguous tensor (copies of any dtype, the unsigned ones included)"""
    torch, _ = _dev()
    assert t.is_contiguous()
    return t.reshape(-1).view(torch.uint8)


class Harness:
    """decoy: the decoy arrays of a helper's inputs, in the order in which the helper arms them (None: that input is not armed).
    wrong_stream: test-only switch — `s` is armed as always, the entry gets the null stream (test_the_harness_detects_a_wrong_stream).
    stream / delay / sync / gate: for the interleaving tests, which put several helpers' calls on two streams one right after
    the other — a harness on a given stream, without a delay, without the device-wide wait in front of the call (that wait
    would outlast the other stream's delay), and with restore() held at `gate` until every call has been made."""
    armed = True

    def __init__(self, decoy=None, wrong_stream=False, stream=None, delay=True, sync=True, gate=None):
        torch, dev = _dev()
        self.decoy = decoy
        self.wrong_stream = wrong_stream
        self.delay, self.sync, self.gate = delay, sync, gate
        self.s = stream if stream is not None else side_stream()
        self.inputs, self.outputs, self.guarded = [], [], []
        self.fired = 0
        self.pending = []                 # per call: was `s` still busy when the entry returned?
        if delay:
            calibrate()

    # ---- inputs
    def arm(self, tensors, decoys=None):
        """the device tensors (or views) hold the real inputs: remember them, leave the decoys in their place"""
        torch, dev = _dev()
        decoys = self.decoy if decoys is None else decoys
        if decoys is None:
            return
        assert len(tensors) == len(decoys), "one decoy (or None) per input"
        for t, d in zip(tensors, decoys):
            if t is None or d is None or np.size(d) == 0:
                continue
            d = np.ascontiguousarray(d, dtype=torch.empty(0, dtype=t.dtype).numpy().dtype)      # as the helper uploaded the real one
            flat = _bytes(t)
            image = torch.from_numpy(d.reshape(-1).view(np.uint8)).to(dev)
            assert image.numel() == flat.numel(), "a decoy has the length and dtype of the real array"
            real = flat.clone()
            flat.copy_(image)
            for x in (t, real, image):     # allocated on torch's current stream, used on `s`: not handed out again before `s` is done
                x.record_stream(self.s)
            self.inputs.append((flat, real, image))

    def up(self, real, decoy):
        torch, dev = _dev()
        t = torch.from_numpy(np.ascontiguousarray(real)).to(dev)
        self.arm([t], [decoy])
        return t

    # ---- outputs
    def watch(self, *tensors):
        """output buffers as the helper filled them (sentinels and guards): the delayed fill writes that image again"""
        for t in tensors:
            if t is not None:
                flat = _bytes(t)
                image = flat.clone()
                t.record_stream(self.s)
                image.record_stream(self.s)
                self.outputs.append((flat, image))

    def out(self, dtype, n, fill):
        """n elements between two guards of 16 bytes (the payload keeps the alignment of the allocation, which kernels that
        store four values at a time need), all `fill` -> the buffer; payload() cuts the guards off and checks them"""
        torch, dev = _dev()
        g = self._guard(np.dtype(dtype).itemsize)
        buf = torch.from_numpy(np.full(n + 2 * g, fill, dtype)).to(dev)
        self.watch(buf)
        self.guarded.append((buf, np.asarray(fill, dtype)))
        return buf

    def retire(self, *tensors):
        """these outputs hold the results of a call that has been made: later calls of the same harness leave them alone"""
        gone = {t.data_ptr() for t in tensors}
        self.outputs = [(flat, image) for flat, image in self.outputs if flat.data_ptr() not in gone]

    @staticmethod
    def _guard(itemsize):
        return max(16 // itemsize, 1)

    @classmethod
    def ptr(cls, buf):
        return buf.data_ptr() + cls._guard(buf.element_size()) * buf.element_size()

    def payload(self, buf):
        a = buf.cpu().numpy()
        fill = next(f for b, f in self.guarded if b is buf)
        g = self._guard(a.itemsize)
        assert (a[:g] == fill).all() and (a[len(a) - g:] == fill).all(), \
            f"write outside an output: {a[:g].tolist()} in front, {a[len(a) - g:].tolist()} behind, {fill} expected"
        return a[g:len(a) - g]

    # ---- the call
    def fire(self):
        """delay, real inputs over the decoys, sentinels over the outputs, all on `s` -> the stream to hand to the entry"""
        torch, _ = _dev()
        if self.fired:
            self._decoys_back()
        if self.sync:
            torch.cuda.synchronize()
        else:                              # the uploads and fills that the helper queued on torch's current stream have landed
            torch.cuda.current_stream().synchronize()
        with torch.cuda.stream(self.s):
            if self.delay:
                _spin(_CAL["units"])
            for flat, real, _ in self.inputs:
                flat.copy_(real)
            for flat, image in self.outputs:
                flat.copy_(image)
        if self.delay:
            assert not self.s.query(), "the delay ended before the entry was called: the call would prove nothing"
        self.fired += 1
        return None if self.wrong_stream else self.s.cuda_stream

    def call(self, fn, *args):
        """arm anew and call fn(*args, stream)"""
        sp = self.fire()
        rc = fn(*args, C.c_void_p(sp))
        self.pending.append(not self.s.query())
        return rc

    def _decoys_back(self):
        torch, _ = _dev()
        with torch.cuda.stream(self.s):
            for flat, _, image in self.inputs:
                flat.copy_(image)
        self.s.synchronize()

    def restore(self):
        """decoys back over the inputs, then wait: the helper downloads its outputs next"""
        torch, _ = _dev()
        if self.gate is not None:
            self.gate.made_its_calls()
        self._decoys_back()
        if self.sync:
            torch.cuda.synchronize()


class Gate:
    """Runs helpers one after the other up to the point where each has made its calls and would wait for its stream
    (Harness.restore), holds them there, and lets them collect their outputs once all have got that far.  Every helper runs in a
    thread of its own, one at a time: nothing here is concurrent on the host."""

    def __init__(self):
        import threading

        self.threading = threading
        self.collect = threading.Event()
        self.local = threading.local()
        self.jobs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.release()

    def made_its_calls(self):
        self.local.launched.set()
        self.collect.wait()

    def start(self, fn, *args, **kw):
        """run fn(*args, **kw) until its harness reaches restore() (or fn ends) -> the job; result() after release()"""
        launched, box = self.threading.Event(), {}

        def body():
            self.local.launched = launched
            try:
                box["value"] = fn(*args, **kw)
            except BaseException as e:           # handed to the test's thread by result()
                box["error"] = e
            launched.set()

        th = self.threading.Thread(target=body, daemon=True)
        th.start()
        launched.wait()
        self.jobs.append((th, box))
        return len(self.jobs) - 1

    def release(self):
        self.collect.set()
        for th, _ in self.jobs:
            th.join()

    def result(self, job):
        box = self.jobs[job][1]
        if "error" in box:
            raise box["error"]
        return box["value"]


# ---------------------------------------------------------------------------------------------------------- decoys (numpy)
def rev_off(off):
    """offsets of the same counts in reverse order: monotone from 0 to the same total"""
    off = np.asarray(off)
    out = np.zeros_like(off)
    np.cumsum(np.diff(off)[::-1], out=out[1:])
    return out


def merge_off(off):
    """offsets of the counts added up in pairs (c0 + c1, 0, c2 + c3, 0, ...): the same total, another distribution of row
    lengths — for a step that counts rows by their length, which a reversed list leaves as it is"""
    c = np.diff(np.asarray(off)).copy()
    m = len(c) // 2 * 2
    c[0:m:2] += c[1:m:2]
    c[1:m:2] = 0
    out = np.zeros_like(np.asarray(off))
    np.cumsum(c, out=out[1:])
    return out


def rev(a):
    return None if a is None else np.ascontiguousarray(np.asarray(a)[::-1])


def moved(xy, width=2, by=(3.25, -1.75)):
    """the points (rows of `width` values) in reverse order and shifted; NaN and inf stay what they are"""
    a = np.asarray(xy, np.float64).reshape(-1, width)[::-1] + np.resize(np.asarray(by, np.float64), width)
    return np.ascontiguousarray(a).reshape(np.shape(xy))


def rot_cls(cls, n_classes):
    """class ids rotated inside 0..n_classes-1; ids outside that range (-1: unmatched) stay"""
    cls = np.asarray(cls)
    ok = (cls >= 0) & (cls < n_classes)
    return np.where(ok, (cls + 1) % max(n_classes, 1), cls).astype(cls.dtype)


def box_table_decoy(box4, row_off, cls, W, H, status, n_classes):
    """K10 / K11's table: boxes reversed and shifted, the rows' counts merged in pairs (K10 counts rows by their length),
    classes rotated, the rows' sizes in reverse order"""
    return moved(box4, 4), merge_off(row_off), rot_cls(cls, n_classes), rev(W), rev(H), rev(status)


def poly_table_decoy(xy, pt_off, row_off, W, H):
    """the polygon steps' table: points reversed and shifted, both count lists reversed, the rows' sizes in reverse order"""
    return moved(xy), rev_off(pt_off), rev_off(row_off), rev(W), rev(H)


def valid_offsets(real, decoy):
    real, decoy = np.asarray(real), np.asarray(decoy)
    return (decoy.dtype == real.dtype and decoy.shape == real.shape and decoy[0] == 0 and (np.diff(decoy) >= 0).all()
            and decoy[-1] == real[-1])


def differs(a, b):
    """two reference outputs (arrays or bytes) differ somewhere; NaN equals NaN"""
    if isinstance(a, (bytes, bytearray)):
        return bytes(a) != bytes(b)
    a, b = np.asarray(a), np.asarray(b)
    return a.shape != b.shape or not np.array_equal(a, b, equal_nan=a.dtype.kind == "f")
