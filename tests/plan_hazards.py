"""What a plan's launches touch, and when they run relative to each other: the support of tests/test_plan_streams_host.py (CPU)
and tests/test_plan_streams_gpu.py.  Not a test file.

  Registry      every allocation reachable from a plan (its own buffers, every op and BatchNorm member, the ParamStore arenas, the
                Comm), by address; views of one storage are one entry; device tables carry the ctypes struct they hold.
  scan          the allocations a launch POINTS at: every integer of `args`, of the structs passed by reference, of the entries of
                the device tables among them.  Values below 2**32 are sizes.
  norm          a declared access (engine.Launch.reads / .writes) as bytes of its allocation.
  record        one call of the real Plan.run_backward as a trace -- launch / record / wait_event / wait_stream / ready -- with
                fake streams and events and a timer hook that records in place of launching.
  Order         happens-before over a trace: vector clocks, one component per stream.
  the checks    completeness, unordered conflicts, closure of the pass, gend, the grad_ready promise: each returns a list of
                findings (strings that name the launches); an empty list is a pass.
  launch_digest name, kernel, arguments and gend of every launch of a plan as a hash that does not depend on addresses.
"""
import bisect
import contextlib
import ctypes as C

import torch

from dualvar_amd import _lib as L
from dualvar_amd import engine, ops

POINTER_MIN = 1 << 32
TABLES = {'_items': L.BnItem, '_ft': L.GemmDesc, '_bt': L.GemmDesc, '_pack_descs': L.PackDesc}      # attribute -> struct of its entries


def label(l):
    return '%s[%s %s]' % (l.name, l.kname, getattr(l, 'shape', ''))


# ------------------------------------------------------------------------------------------------------------ allocations
class Alloc:
    def __init__(self, name, tensor, struct):
        st = tensor.untyped_storage()
        self.name, self.base, self.nbytes, self.struct, self.tensor = name, st.data_ptr(), st.nbytes(), struct, tensor

    def bytes(self):
        """the whole storage as a uint8 tensor (a view: writing it writes the allocation)"""
        return torch.empty(0, dtype=torch.uint8, device=self.tensor.device).set_(self.tensor.untyped_storage())

    def entries(self):
        raw = bytes(self.bytes().cpu().numpy())
        n = len(raw) // C.sizeof(self.struct)
        return (self.struct * n).from_buffer_copy(raw[:n * C.sizeof(self.struct)])

    def __repr__(self):
        return self.name


class Registry:
    def __init__(self, plan, extra=()):
        self.by_base, self._seen = {}, set()
        self._walk(plan, 'plan')
        for name, t in extra:
            self._walk(t, name)
        self._bases = sorted(self.by_base)

    def _add(self, t, name, attr):
        st = t.untyped_storage()
        if st.nbytes() == 0:
            return
        a = self.by_base.get(st.data_ptr())
        if a is None:
            self.by_base[st.data_ptr()] = Alloc(name, t, TABLES.get(attr))
        elif a.struct is None and attr in TABLES:
            a.struct, a.name = TABLES[attr], name

    def _walk(self, o, name, attr=None):
        if isinstance(o, torch.Tensor):
            return self._add(o, name, attr)
        if o is None or isinstance(o, (int, float, str, bytes, bool, C.Structure, C.CDLL)) or id(o) in self._seen:
            return
        if hasattr(o, 'kname') or isinstance(o, engine.PairMember):      # a launch's declared sets register nothing: they are checked
            return
        self._seen.add(id(o))
        if isinstance(o, dict):
            for k, v in o.items():
                self._walk(v, '%s.%s' % (name, k), k if isinstance(k, str) else None)
        elif isinstance(o, (list, tuple, set)):
            for i, v in enumerate(o):
                self._walk(v, '%s[%d]' % (name, i), attr)
        elif isinstance(o, torch.nn.Module) or type(o).__module__.startswith('dualvar_amd'):
            fields = dict(getattr(o, '__dict__', {}))
            for cls in type(o).__mro__:
                for s in getattr(cls, '__slots__', ()):
                    if hasattr(o, s):
                        fields[s] = getattr(o, s)
            tag = type(o).__name__
            for k, v in fields.items():
                self._walk(v, '%s:%s.%s' % (name, tag, k) if name.count('.') < 3 else '%s.%s' % (tag, k), k)

    def find(self, addr):
        i = bisect.bisect_right(self._bases, addr) - 1
        if i >= 0:
            a = self.by_base[self._bases[i]]
            if addr < a.base + a.nbytes:
                return a
        return None


def _ints(obj):
    """the integer fields of a ctypes struct"""
    for f in obj._fields_:
        v = getattr(obj, f[0])
        if isinstance(v, int) and not isinstance(v, bool):
            yield v


def scan(reg, l):
    """{allocation: [addresses]} a launch points at -- through its arguments, the structs it passes and the tables among them"""
    found, todo = {}, []
    for a in getattr(l, 'args', ()):
        if isinstance(a, int) and not isinstance(a, bool):
            todo.append(a)
        elif hasattr(a, '_obj') and isinstance(a._obj, C.Structure):
            todo += list(_ints(a._obj))
    while todo:
        v = todo.pop()
        if v < POINTER_MIN:
            continue
        a = reg.find(v)
        if a is None:
            continue
        if a not in found and a.struct is not None:
            for e in a.entries():
                todo += list(_ints(e))
        found.setdefault(a, []).append(v)
    return found


# ------------------------------------------------------------------------------------------------------------ accesses
class Span:
    """a declared access inside its allocation, in bytes: [lo, hi) overall; for an activation also the row pitch, the first row's
    start and the column bytes [c0, c1) of every row"""
    __slots__ = ('alloc', 'lo', 'hi', 'ld', 'row0', 'c0', 'c1', 'rows')

    def overlaps(self, o):
        if self.alloc is not o.alloc or self.lo >= o.hi or o.lo >= self.hi:
            return False
        if self.ld and self.ld == o.ld and self.row0 == o.row0:      # two views of the same rows: compare the columns
            return self.c0 < o.c1 and o.c0 < self.c1
        # two activations of different pitch (a reshaped view): the whole allocation, conservatively; a flat range against rows,
        # or two flat ranges: the envelopes, which have just been compared
        return True

    def mask(self, m):
        """set this access in a bool mask over the allocation's bytes"""
        if self.ld:
            m[self.row0:self.row0 + self.rows * self.ld].view(self.rows, self.ld)[:, self.c0:self.c1] = True
        else:
            m[self.lo:self.hi] = True


def norm(reg, acc):
    """-> Span of one access; raises LookupError if it is not inside a registered allocation"""
    s = Span()
    if isinstance(acc, ops.Act):
        es, t = ops.ESIZE[acc.dtype], acc.buf
        a = reg.find(t.data_ptr()) if t.untyped_storage().nbytes() else None
        if a is None:
            raise LookupError('activation buffer %r is not registered' % (tuple(t.shape),))
        s.alloc, s.ld, s.rows, s.row0 = a, acc.ld * es, acc.rows, t.data_ptr() - a.base
        s.c0, s.c1 = acc.off * es, min(acc.off + acc.cpitch, acc.ld) * es
        s.lo, s.hi = s.row0 + s.c0, s.row0 + (s.rows - 1) * s.ld + s.c1
    else:
        t, first, end = acc
        es = t.element_size()
        a = reg.find(t.data_ptr()) if t.untyped_storage().nbytes() else None
        if a is None:
            raise LookupError('tensor %r is not registered' % (tuple(t.shape),))
        s.alloc, s.ld, s.rows, s.row0, s.c0, s.c1 = a, 0, 0, 0, 0, 0
        s.lo, s.hi = t.data_ptr() - a.base + first * es, t.data_ptr() - a.base + end * es
    if not (0 <= s.lo < s.hi <= s.alloc.nbytes):
        raise LookupError('access [%d, %d) leaves %s (%d bytes)' % (s.lo, s.hi, s.alloc.name, s.alloc.nbytes))
    return s


class Sets:
    """the normalised reads and writes of launches, computed once per launch"""

    def __init__(self, reg):
        self.reg, self._c = reg, {}

    def __call__(self, l):
        e = self._c.get(id(l))
        if e is None:
            e = self._c[id(l)] = (l, [norm(self.reg, a) for a in l.reads], [norm(self.reg, a) for a in l.writes])
        return e[1], e[2]


def launches(plan):
    return list(plan.f_list) + list(plan.b_list)


def check_complete(plan, reg, lists=None):
    """every allocation a launch points at is among its declared accesses; every declared access lies in a registered allocation"""
    bad = []
    for l in (launches(plan) if lists is None else lists):
        try:
            spans = [norm(reg, a) for a in tuple(l.reads) + tuple(l.writes)]
        except LookupError as e:
            bad.append('%s declares an access outside the plan: %s' % (label(l), e))
            continue
        declared = {s.alloc for s in spans}
        for a, addrs in scan(reg, l).items():
            if a not in declared:
                bad.append('%s points into %s (0x%x) and declares neither a read nor a write of it' % (label(l), a.name, addrs[0]))
            else:
                for v in addrs:
                    if not any(s.alloc is a and s.lo <= v - a.base < s.hi for s in spans):
                        bad.append('%s points at %s+%d, outside every range it declares there' % (label(l), a.name, v - a.base))
    return bad


def grad_spans(sets, l, grad_alloc, writes_only=False):
    r, w = sets(l)
    return [s for s in (w if writes_only else r + w) if s.alloc is grad_alloc]


def check_gend(plan, reg, sets, lists=None):
    """Launch.gend is the largest end (elements) among the launch's declared writes into the gradient arena; 0 if it writes none"""
    g = reg.find(plan.store.grad.data_ptr())
    bad = []
    for l in (launches(plan) if lists is None else lists):
        ends = [s.hi // 4 for s in grad_spans(sets, l, g, writes_only=True)]
        if getattr(l, 'gend', 0) != max(ends + [0]):
            bad.append('%s has gend %d and writes the gradient arena up to %d' % (label(l), getattr(l, 'gend', 0), max(ends + [0])))
    return bad


# ------------------------------------------------------------------------------------------------------------ the trace
class FakeStream:
    _next = [0x7000]

    def __init__(self, rec, name):
        self.rec, self.name = rec, name
        FakeStream._next[0] += 0x10
        self.cuda_stream = FakeStream._next[0]
        rec.streams[self.cuda_stream] = self

    def wait_event(self, ev):
        self.rec.trace.append(('wait_event', self, ev))

    def wait_stream(self, other):
        self.rec.trace.append(('wait_stream', self, other))

    def __repr__(self):
        return self.name


class FakeEvent:
    def __init__(self, rec):
        self.rec = rec

    def record(self, stream=None):
        self.rec.trace.append(('record', self, stream if stream is not None else self.rec.main))


class Recorder:
    """trace: ('launch', stream, l) | ('record', event, stream) | ('wait_event', stream, event) | ('wait_stream', a, b) |
    ('ready', lo)"""

    def __init__(self):
        self.trace, self.streams, self.exchange = [], {}, None
        self.main = FakeStream(self, 'main')

    def timer(self, l, s, stream=None):
        st = self.streams[s]
        if l.name == 'syncbn_allreduce_start':
            # the asynchronous all-reduce of a torch.distributed backend on a device runs on the communicator's own stream, behind
            # what the calling stream holds at the call -- the third stream of a world > 1 backward
            if self.exchange is None:
                self.exchange = FakeStream(self, 'exchange')
            ev = FakeEvent(self)
            ev.record(st)
            self.exchange.wait_event(ev)
            st = self.exchange
        elif l.name == 'syncbn_allreduce_wait':      # work.wait(): the calling stream waits for the collective
            ev = FakeEvent(self)
            ev.record(self.exchange)
            st.wait_event(ev)
        self.trace.append(('launch', st, l))

    def ready(self, plan, lo):
        self.trace.append(('ready', lo))


@contextlib.contextmanager
def fake_streams(rec):
    saved = (torch.cuda.current_stream, torch.cuda.Stream, torch.cuda.Event)
    n = [0]

    def new_stream(*a, **k):
        n[0] += 1
        return FakeStream(rec, 'side' if n[0] == 1 else 'stream%d' % n[0])
    torch.cuda.current_stream = lambda *a, **k: rec.main
    torch.cuda.Stream = new_stream
    torch.cuda.Event = lambda *a, **k: FakeEvent(rec)
    try:
        yield
    finally:
        torch.cuda.current_stream, torch.cuda.Stream, torch.cuda.Event = saved


def record(plan, armed=False, bucket_starts=()):
    """one call of the plan's own run_backward -> Recorder.  Nothing is launched.  The plan's streams, events, timer and
    grad_ready hook are put back."""
    rec = Recorder()
    saved = (plan._side, plan._events, plan.timer, plan.grad_ready, plan.bucket_starts, plan._triggers)
    plan._side = plan._events = plan._triggers = None
    plan.timer, plan.grad_ready, plan.bucket_starts = rec.timer, (rec.ready if armed else None), tuple(bucket_starts)
    try:
        with fake_streams(rec):
            plan.run_backward()
    finally:
        plan._side, plan._events, plan.timer, plan.grad_ready, plan.bucket_starts, plan._triggers = saved
    return rec


class Node:
    __slots__ = ('pos', 'stream', 'launch', 'vc', 'lo')


class Order:
    """Happens-before over a trace.  Every stream has a clock vector with one component per stream; a launch ticks its stream's own
    component and takes the vector as its time; record copies the stream's vector into the event; wait_event / wait_stream take
    the component-wise maximum.  A happens-before B iff B's vector has reached A's own component.  A ready(lo) node joins every
    stream but a third one (what GradSync's communication stream waits for: the main and the side stream) and orders nothing
    after it."""

    def __init__(self, trace, drop=()):
        self.idx, self.nodes, self.ready = {}, [], []
        clock, evs = {}, {}

        def clk(s):
            if s not in self.idx:
                self.idx[s] = len(self.idx)
            return clock.setdefault(s, {})

        def join(a, b):
            for k, v in b.items():
                if a.get(k, 0) < v:
                    a[k] = v
        for pos, step in enumerate(trace):
            kind = step[0]
            if kind in drop:
                continue
            if kind == 'launch':
                c = clk(step[1])
                c[step[1]] = c.get(step[1], 0) + 1
                n = Node()
                n.pos, n.stream, n.launch, n.vc, n.lo = pos, step[1], step[2], dict(c), None
                self.nodes.append(n)
            elif kind == 'record':
                evs[id(step[1])] = dict(clk(step[2]))
            elif kind == 'wait_event':
                join(clk(step[1]), evs.get(id(step[2]), {}))
            elif kind == 'wait_stream':
                join(clk(step[1]), clk(step[2]))
            elif kind == 'ready':
                n = Node()
                n.pos, n.stream, n.launch, n.vc, n.lo = pos, None, None, {}, step[1]
                for s, c in clock.items():
                    if s.name in ('main', 'side'):
                        join(n.vc, c)
                self.ready.append(n)
        self.end = {s: dict(c) for s, c in clock.items()}

    @staticmethod
    def before(a, b_vc):
        """launch node a happens-before the point whose vector is b_vc"""
        return b_vc.get(a.stream, 0) >= a.vc[a.stream]


def check_conflicts(order, sets, lst):
    """Two launches with a conflicting access pair -- one allocation, overlapping ranges, at least one a write -- must be ordered,
    and in the order of the list `lst` the plan was written in: the earlier one happens-before the later one.  (A deferred side
    launch that a later main-stream launch overtakes IS ordered -- the wrong way round.)
    -> [(first node, second node, text)]"""
    place = {id(l): i for i, l in enumerate(lst)}
    per = {}
    for n in order.nodes:
        r, w = sets(n.launch)
        for s in r:
            per.setdefault(s.alloc, []).append((n, s, False))
        for s in w:
            per.setdefault(s.alloc, []).append((n, s, True))
    bad, seen = [], set()
    for alloc, lst in per.items():
        if not any(wr for _, _, wr in lst):
            continue
        for i, (na, sa, wa) in enumerate(lst):
            for nb, sb, wb in lst[i + 1:]:
                if na is nb or na.stream is nb.stream or not (wa or wb) or (na.pos, nb.pos) in seen:
                    continue
                if not sa.overlaps(sb):
                    continue
                first, second = (na, nb) if place[id(na.launch)] < place[id(nb.launch)] else (nb, na)
                if order.before(first, second.vc):
                    continue
                seen.add((na.pos, nb.pos))
                how = 'runs BEFORE it' if order.before(second, first.vc) else 'is not ordered with it'
                bad.append((first, second, '%s on %s (list position %d, %s of %s) must happen before %s on %s (position %d, %s), which %s' % (
                    label(first.launch), first.stream, place[id(first.launch)], 'write' if (wa if first is na else wb) else 'read',
                    alloc.name, label(second.launch), second.stream, place[id(second.launch)],
                    'write' if (wb if first is na else wa) else 'read', how)))
    bad.sort(key=lambda t: (place[id(t[0].launch)], place[id(t[1].launch)]))
    return bad


def flagged(order, sets, conflicts):
    """the launches of `conflicts`, and those that conflict with an earlier flagged launch of their own stream (they run on what
    the race left): {id(launch)}"""
    out = {id(n.launch) for a, b, _ in conflicts for n in (a, b)}
    hit = [n for n in order.nodes if id(n.launch) in out]
    for n in order.nodes:
        if id(n.launch) in out:
            continue
        r, w = sets(n.launch)
        for m in hit:
            if m.stream is n.stream and m.pos < n.pos:
                mr, mw = sets(m.launch)
                if any(a.overlaps(b) for a in w for b in mr + mw) or any(a.overlaps(b) for a in r for b in mw):
                    out.add(id(n.launch))
                    hit.append(n)
                    break
    return out


def check_closed(rec, order):
    """the last step is the main stream's wait for the side stream, and every launch happens-before the end of the pass"""
    bad = []
    last = rec.trace[-1] if rec.trace else None
    side = [s for s in rec.streams.values() if s is not rec.main]
    if side and not (last and last[0] == 'wait_stream' and last[1] is rec.main and last[2].name == 'side'):
        bad.append('the pass does not end with the main stream waiting for the side stream')
    end = order.end.get(rec.main, {})
    for n in order.nodes:
        if not order.before(n, end):
            bad.append('%s on %s is not ordered before the end of the pass' % (label(n.launch), n.stream))
    return bad


def check_ready(plan, reg, order, sets):
    """at ready(lo): every launch that touches the gradient arena at or above element lo happens-before the node, and none
    comes after it in the trace"""
    g = reg.find(plan.store.grad.data_ptr())
    off = plan.store.grad.data_ptr() - g.base
    bad = []
    for r in order.ready:
        for n in order.nodes:
            if not any(s.hi > off + 4 * r.lo for s in grad_spans(sets, n.launch, g)):
                continue
            if n.pos > r.pos:
                bad.append('%s touches the gradient arena at or above %d after ready(%d)' % (label(n.launch), r.lo, r.lo))
            elif not order.before(n, r.vc):
                bad.append('%s on %s touches the gradient arena at or above %d and is not ordered before ready(%d)' % (
                    label(n.launch), n.stream, r.lo, r.lo))
    return bad


def one_stream_trace(plan):
    """the trace with engine.WGRAD_SIDE_STREAM off"""
    saved = engine.WGRAD_SIDE_STREAM
    engine.WGRAD_SIDE_STREAM = False
    rec = Recorder()
    t, plan.timer = plan.timer, rec.timer
    try:
        with fake_streams(rec):
            plan.run_backward()
    finally:
        engine.WGRAD_SIDE_STREAM, plan.timer = saved, t
    return rec


# ------------------------------------------------------------------------------------------------------------ launch digest
def launch_digest(plan, reg):
    """sha256 over (name, kname, args) of every launch of f_list and b_list, position by position.  Pointers are written as
    (allocation in order of first appearance, offset in it), so two builds of one plan agree exactly when every launch points
    at the same place of the same buffer; struct arguments are written field by field.  None of it looks at reads / writes."""
    import hashlib
    import json
    seen = {}

    def val(v):
        if isinstance(v, bool) or v is None:
            return v
        if isinstance(v, int):
            if v < POINTER_MIN:
                return v
            a = reg.find(v)
            return ['ptr?'] if a is None else ['ptr', seen.setdefault(a.base, len(seen)), v - a.base]
        if isinstance(v, float):
            return repr(v)
        if hasattr(v, '_obj') and isinstance(v._obj, C.Structure):
            return [[f[0], val(getattr(v._obj, f[0]))] for f in v._obj._fields_]
        return str(type(v).__name__)
    out = {}
    for key, lst in (('f', plan.f_list), ('b', plan.b_list)):
        rows = [[l.name, l.kname, [val(a) for a in getattr(l, 'args', ())], getattr(l, 'gend', 0)] for l in lst]
        out[key] = [len(rows), hashlib.sha256(json.dumps(rows).encode()).hexdigest()]
    return out
