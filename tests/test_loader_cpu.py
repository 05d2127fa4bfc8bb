"""Test-set loader (vitcap_amd/loader.py) without a GPU: the decode-ahead plan, the scheduling and slab-reuse rules with a recording
fake executor, the release of every shared-memory segment on each way out, the real worker path with an identity preprocess, and
prefetched() on a CPU device."""
import base64
import gc
import io
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
from multiprocessing import shared_memory

import numpy as np
import pytest
import torch

from vitcap_amd import jpegdec as J
from vitcap_amd import loader as L
from vitcap_amd.tsv import tsv_writer

MB, GB = 1 << 20, 1 << 30


@pytest.fixture(autouse=True)
def _no_page_locking(monkeypatch):
    """The slabs stay pageable here (the page-locking path needs the GPU runtime: tests/test_hip_loader.py); handles that in-process
    worker threads attached (jpegdec._SHM) are dropped afterwards."""
    monkeypatch.setenv('VITCAP_LOADER_PIN', '0')
    yield
    gc.collect()                # a failed task's traceback holds a view of its slab
    for shm in J._SHM.values():
        shm.close()
    J._SHM.clear()


def unlinked(name):
    try:
        shared_memory.SharedMemory(name=name).close()
    except FileNotFoundError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------------- 1. plan
# (bs, workers, chunk, slab bytes, budget bytes, slabs used, VITCAP_LOADER_AHEAD) -> (per_batch, ahead, n_slabs).  The right-hand
# sides were produced by evaluating the expressions of the commit BEFORE loader.py existed (pipeline.py iter_test_batches, copied
# literally into a scratch script: per_batch = (bs + chunk - 1) // chunk; ahead = min(12, max(3, (10 * workers + per_batch - 1) //
# per_batch)); ahead = int(os.environ.get('VITCAP_LOADER_AHEAD', ahead)); with slabs ahead = max(1, min(ahead, budget // (per_batch *
# slab_bytes) - 3)), n_slabs = (ahead + 3) * per_batch), not by calling decode_ahead_plan.
PLAN_TABLE = [
    ((64, 1, 8, 24 * MB, 4 * GB, True, None), (8, 3, 48)),
    ((512, 32, 8, 24 * MB, 4 * GB, True, None), (64, 1, 256)),      # the floor: the budget cannot be met and `ahead` stays 1
    ((2, 1, 8, 24 * MB, 4 * GB, True, None), (1, 10, 13)),
    ((64, 16, 8, 24 * MB, 4 * GB, True, None), (8, 12, 120)),       # the 12 cap
    ((64, 8, 8, 24 * MB, 4 * GB, True, None), (8, 10, 104)),        # the shipped defaults at batch 64
    ((48, 8, 8, 24 * MB, 4 * GB, True, None), (6, 12, 90)),
    ((65, 8, 8, 24 * MB, 4 * GB, True, None), (9, 9, 108)),         # a ragged last chunk counts as a task
    ((256, 8, 8, 24 * MB, 4 * GB, True, None), (32, 2, 160)),       # the byte budget bites
    ((64, 8, 8, 24 * MB, 1 * GB, True, None), (8, 2, 40)),
    ((64, 8, 8, 24 * MB, 4 * GB, False, None), (8, 10, 0)),         # no slabs (threads): no byte cap, no slabs
    ((512, 32, 8, 24 * MB, 4 * GB, False, None), (64, 5, 0)),
    ((64, 8, 8, 24 * MB, 4 * GB, True, '1'), (8, 1, 32)),           # override
    ((64, 8, 8, 24 * MB, 4 * GB, True, '20'), (8, 18, 168)),        # the override passes the 12 cap but not the byte budget
    ((64, 8, 8, 24 * MB, 4 * GB, False, '20'), (8, 20, 0)),
    ((4, 2, 3, 1 * MB, 4 * GB, True, '1'), (2, 1, 8)),              # the shapes of the scheduling tests below
    ((4, 2, 3, 1 * MB, 4 * GB, True, '3'), (2, 3, 12)),
    ((4, 2, 3, 1 * MB, 4 * GB, True, None), (2, 10, 26)),
]


@pytest.mark.parametrize('args,want', PLAN_TABLE)
def test_decode_ahead_plan_matches_the_recorded_table(args, want):
    plan = L.decode_ahead_plan(*args)
    assert tuple(plan) == want
    assert (plan.per_batch, plan.ahead, plan.n_slabs) == want


# ---------------------------------------------------------------------------------------------------------------- 2. scheduling
class FakeFuture(object):
    def __init__(self, ex, task):
        self.ex, self.task = ex, task

    def result(self):
        """Completes on demand: keys 'k<row>'; one 1x1 image per row, inside the slab (offset, h, w) or as an array."""
        t = self.task
        assert not t['collected']
        t['collected'] = True
        keys = ['k%d' % i for i in t['rows']]
        if t['slab'] is None:
            return keys, [np.full((1, 1, 3), i, np.uint8) for i in t['rows']]
        buf = np.frombuffer(self.ex.segments[t['slab']].buf, dtype=np.uint8)
        for j, i in enumerate(t['rows']):
            buf[16 * j:16 * j + 3] = i
        del buf
        return keys, [(16 * j, 1, 1) for j in range(len(t['rows']))]


class FakeExecutor(object):
    """Records every task and checks, at the moment a task is submitted, the rules the loader has to keep."""

    def __init__(self, slabs, ahead, bs, stride):
        self.segments = list(slabs.segments)
        self.names = [s.name for s in self.segments]
        self.ahead, self.bs, self.stride = ahead, bs, stride
        self.tasks, self.handed_out, self.is_shut_down, self.max_inflight = [], [], False, 0

    def submit(self, fn, *args):
        assert not self.is_shut_down
        if fn is J.decode_rows_into:
            name, tsv, rows, device_jpeg = args
            sid = self.names.index(name)
        else:
            assert fn is J.decode_rows
            (tsv, rows), sid = args, None
        first = self.tasks[0]['rows'][0] if self.tasks else rows[0]
        task = {'fn': fn, 'slab': sid, 'rows': list(rows), 'collected': False, 'batch': (rows[0] - first) // self.stride // self.bs, 'tsv': tsv}
        if sid is not None:
            held = {t['slab'] for t in self.tasks if not t['collected']}                                        # uncollected tasks
            held |= {t['slab'] for t in self.tasks if t['collected'] and t['batch'] >= len(self.handed_out)}    # batch being assembled
            held |= {t['slab'] for t in self.tasks if t['batch'] in self.handed_out[-2:]}                       # last two handed out
            assert sid not in held, 'slab %d given to a new task while still held' % sid
        self.tasks.append(task)
        inflight = {t['batch'] for t in self.tasks if not t['collected']}
        self.max_inflight = max(self.max_inflight, len(inflight))
        assert len(inflight) <= self.ahead
        return FakeFuture(self, task)

    def shutdown(self, wait=True):
        self.is_shut_down = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.shutdown()


class CountingSlabPool(L.SlabPool):
    min_free = None

    def take(self):
        assert self.free, 'take() found the free list empty'
        self.min_free = min(len(self.free) - 1, len(self) if self.min_free is None else self.min_free)
        return super().take()


def fake_run(n_rows, ahead, use_slabs=True, world=2, rank=1, bs=4, chunk=3):
    """-> (yielded batches, executor, slab names).  A batch counts as handed out from the moment its images go to the preprocess
    callable (that call enqueues the host -> device copies; the yield follows it with the submission of one more batch in between):
    this is the event the loader's retirement rule counts from."""
    plan = L.decode_ahead_plan(bs, 2, chunk, 4096, 4 * GB, use_slabs, str(ahead))
    assert plan.ahead == ahead
    slabs = CountingSlabPool(plan, 4096)
    assert len(slabs) == plan.n_slabs
    ex = FakeExecutor(slabs, ahead, bs, world)

    def pre(imgs):
        ex.handed_out.append(len(ex.handed_out))
        return [np.array(im) for im in imgs]         # copies: no view of a slab leaves the loader
    rows = list(range(rank, n_rows, world))
    out = list(L.PredictBatchLoader('/no/such.tsv', rows, bs, chunk, plan, ex, slabs, False, pre))
    assert ex.is_shut_down and len(slabs) == 0 and all(t['collected'] for t in ex.tasks)
    assert all(unlinked(n) for n in ex.names)
    return out, ex, slabs


@pytest.mark.parametrize('ahead', [1, 3])
@pytest.mark.parametrize('use_slabs', [True, False], ids=['slabs', 'pipe'])
def test_scheduling_order_depth_and_slab_reuse(ahead, use_slabs):
    """23 rows, world 2, rank 1 -> rows 1, 3, ..., 21 in batches of 4, 4, 3 = tasks of 3+1, 3+1, 3 rows.  The rules themselves are
    asserted by FakeExecutor.submit (depth, slab reuse) and CountingSlabPool.take (free list never empty with the plan's n_slabs)."""
    out, ex, slabs = fake_run(23, ahead, use_slabs)
    want_rows = list(range(1, 23, 2))
    assert [t['rows'] for t in ex.tasks] == [[1, 3, 5], [7], [9, 11, 13], [15], [17, 19, 21]]
    assert [len(b['key']) for b in out] == [4, 4, 3]
    assert [k for b in out for k in b['key']] == ['k%d' % i for i in want_rows]
    assert [int(im[0, 0, 0]) for b in out for im in b['image']] == want_rows
    assert all((t['fn'] is J.decode_rows_into) == use_slabs for t in ex.tasks)
    assert ex.max_inflight == min(ahead, 3)


@pytest.mark.parametrize('ahead', [1, 3])
def test_slabs_are_recycled_over_a_long_run(ahead):
    """16 batches: every slab is taken again several times; the reuse rule is asserted at every submission."""
    out, ex, slabs = fake_run(61, ahead, world=1, rank=0)
    assert [k for b in out for k in b['key']] == ['k%d' % i for i in range(61)]
    assert [int(im[0, 0, 0]) for b in out for im in b['image']] == list(range(61))
    assert len(ex.tasks) == 31 > len(ex.names) and ex.max_inflight == ahead
    assert slabs.min_free is not None and slabs.min_free >= 0


@pytest.mark.parametrize('use_slabs', [True, False], ids=['slabs', 'pipe'])
def test_zero_rows_yield_nothing_and_leak_nothing(use_slabs):
    out, ex, slabs = fake_run(1, 3, use_slabs)          # rank 1 of 2 has no row of a one-row file
    assert out == [] and ex.tasks == []
    assert len(ex.names) == (12 if use_slabs else 0)


def test_close_before_the_first_batch_releases_everything():
    plan = L.decode_ahead_plan(4, 2, 3, 4096, 4 * GB, True, '1')
    slabs = L.SlabPool(plan, 4096)
    ex = FakeExecutor(slabs, 1, 4, 1)
    ld = L.PredictBatchLoader('/no/such.tsv', [0, 1, 2], 4, 3, plan, ex, slabs, False, list)
    ld.close()
    assert ex.is_shut_down and ex.tasks == [] and all(unlinked(n) for n in ex.names)
    assert list(ld) == []


# ---------------------------------------------------------------------------------------------------------------- toy TSV
def _jpeg(h, w, seed, **kw):
    from PIL import Image
    g = np.random.default_rng(seed)
    base = g.integers(0, 256, size=(h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    arr = np.asarray(Image.fromarray(base, 'RGB').resize((w, h), Image.BILINEAR))
    buf = io.BytesIO()
    Image.fromarray(arr, 'RGB').save(buf, format='JPEG', quality=90, **kw)
    return base64.b64encode(buf.getvalue())


TOY_SIZES = [(48, 64), (33, 50), (64, 48), (700, 700), (17, 23), (40, 40)]      # 700x700: 1.4 MB of pixels, does not fit a 1 MiB slab


@pytest.fixture(scope='module')
def toy(tmp_path_factory):
    """-> (tsv path, rows, decode_image of every row): five small JPEGs and one that does not fit a 1 MiB slab."""
    d = tmp_path_factory.mktemp('toy')
    rows = [('img%d' % i, _jpeg(h, w, 10 + i)) for i, (h, w) in enumerate(TOY_SIZES)]
    tsv_writer(rows, str(d / 'test.tsv'))
    want = [J.decode_image(r[1]) for r in rows]
    for a in want:
        a.setflags(write=False)
    return str(d / 'test.tsv'), rows, want


def identity(imgs):
    """Preprocess stand-in: private copies of what the loader assembled (a CoefImage as (info bytes, coefficients))."""
    return [np.array(im) if isinstance(im, np.ndarray) else (bytes(im.info), np.array(im.coefs)) for im in imgs]


def toy_loader(tsv, n_rows, executor, use_slabs=True, device_jpeg=False, ahead='1'):
    plan = L.decode_ahead_plan(4, 2, 3, 1 * MB, 4 * GB, use_slabs, ahead)
    slabs = L.SlabPool(plan, 1 * MB)
    assert len(slabs) == plan.n_slabs
    names = [s.name for s in slabs.segments]
    return L.PredictBatchLoader(tsv, list(range(n_rows)), 4, 3, plan, executor, slabs, device_jpeg, identity), names


def is_shut_down(executor):
    with pytest.raises(RuntimeError):
        executor.submit(int)
    return True


# ---------------------------------------------------------------------------------------------------------------- 3. cleanup
def test_cleanup_on_exhaustion(toy):
    tsv, rows, want = toy
    ex = ThreadPoolExecutor(2)
    ld, names = toy_loader(tsv, len(rows), ex)
    assert len(names) == 8 and not any(unlinked(n) for n in names)
    out = list(ld)
    assert [k for b in out for k in b['key']] == [r[0] for r in rows]
    assert all(unlinked(n) for n in names) and is_shut_down(ex)


def test_cleanup_on_close_after_the_first_batch(toy):
    tsv, rows, want = toy
    ex = ThreadPoolExecutor(2)
    ld, names = toy_loader(tsv, len(rows), ex, ahead='3')
    first = next(ld)
    assert first['key'] == [r[0] for r in rows[:4]] and not any(unlinked(n) for n in names)
    ld.close()
    assert all(unlinked(n) for n in names) and is_shut_down(ex)
    assert list(ld) == []


@pytest.mark.parametrize('use_slabs', [True, False], ids=['slabs', 'pipe'])
def test_cleanup_when_a_task_raises(toy, tmp_path, use_slabs):
    """Row 5 of 7 is not an image: the worker's exception reaches the consumer after the first batch, and everything is released."""
    from PIL import UnidentifiedImageError
    tsv, rows, want = toy
    bad = rows[:5] + [('broken', base64.b64encode(b'this is not an image'))] + rows[5:]
    tsv_writer(bad, str(tmp_path / 'bad.tsv'))
    ex = ThreadPoolExecutor(2)
    ld, names = toy_loader(str(tmp_path / 'bad.tsv'), len(bad), ex, use_slabs)
    assert next(ld)['key'] == [r[0] for r in bad[:4]]
    with pytest.raises(UnidentifiedImageError):
        next(ld)
    assert all(unlinked(n) for n in names) and is_shut_down(ex)
    with pytest.raises(StopIteration):
        next(ld)


# ---------------------------------------------------------------------------------------------------------------- 4. real path
def spawned_pool():
    return L.decode_executor(2)


def test_decode_executor_kinds():
    ex = L.decode_executor(2, threads=True)
    assert isinstance(ex, ThreadPoolExecutor)
    ex.shutdown()
    ex = spawned_pool()
    assert isinstance(ex, ProcessPoolExecutor) and ex._mp_context.get_start_method() == 'spawn'
    ex.shutdown()


def check_pixels(out, rows, want):
    assert [k for b in out for k in b['key']] == [r[0] for r in rows]
    got = [im for b in out for im in b['image']]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.shape == w.shape and np.array_equal(g, w)


@pytest.mark.parametrize('use_slabs', [True, False], ids=['slabs', 'pipe'])
def test_spawned_workers_decode_the_rows(toy, use_slabs):
    """Two spawned worker processes; the 700x700 image does not fit its 1 MiB slab and comes back through the pipe."""
    tsv, rows, want = toy
    ld, names = toy_loader(tsv, len(rows), spawned_pool(), use_slabs)
    check_pixels(list(ld), rows, want)
    assert all(unlinked(n) for n in names)


@pytest.mark.skipif(J.jpeg_lib() is None, reason='libvitcap_jpeg.so not built')
def test_spawned_workers_entropy_decode_only_with_device_jpeg(toy):
    """device_jpeg: a baseline JPEG that fits the slab arrives as a CoefImage with decode_coefs' JpegInfo and coefficients; the oversize
    one (1.5 MB of coefficients, 1.4 MB of pixels) still arrives as Pillow's pixels through the pipe."""
    tsv, rows, want = toy
    ld, names = toy_loader(tsv, len(rows), spawned_pool(), device_jpeg=True)
    out = list(ld)
    assert [k for b in out for k in b['key']] == [r[0] for r in rows]
    got = [im for b in out for im in b['image']]
    for i, (g, r) in enumerate(zip(got, rows)):
        if TOY_SIZES[i] == (700, 700):
            assert np.array_equal(g, want[i])
            continue
        info, coefs = J.decode_coefs(r[1])
        assert isinstance(g, tuple) and g[0] == bytes(info) and g[1].dtype == np.int16 and np.array_equal(g[1], coefs)
    assert all(unlinked(n) for n in names)


@pytest.mark.parametrize('use_slabs', [False, True], ids=['pipe', 'slabs'])
def test_threads_decode_the_rows(toy, use_slabs):
    """`loader_threads: true` runs the same tasks in threads of this process (the pipeline then plans without slabs)."""
    tsv, rows, want = toy
    ld, names = toy_loader(tsv, len(rows), L.decode_executor(2, threads=True), use_slabs, ahead='3')
    check_pixels(list(ld), rows, want)
    assert all(unlinked(n) for n in names)


# ---------------------------------------------------------------------------------------------------------------- 5. prefetched
CPU = torch.device('cpu')


def test_prefetched_keeps_the_order():
    assert list(L.prefetched(iter(range(50)), CPU, depth=3)) == list(range(50))
    assert list(L.prefetched(iter(()), CPU)) == []


def test_prefetched_raises_the_generators_exception_in_the_consumer():
    def gen():
        yield 1
        yield 2
        raise KeyError('from the producer')
    got = []
    with pytest.raises(KeyError, match='from the producer'):
        for b in L.prefetched(gen(), CPU):
            got.append(b)
    assert got == [1, 2]


@pytest.mark.parametrize('depth', [1, 4])
def test_prefetched_consumer_stops_early(depth):
    """The generator's own `finally` (the loader's executor and slabs) has run by the time prefetched() returns."""
    state = {'finalised': False, 'made': 0}

    def gen():
        try:
            for i in range(1000):
                state['made'] = i + 1
                yield i
        finally:
            state['finalised'] = True
    p = L.prefetched(gen(), CPU, depth=depth)
    assert next(p) == 0 and next(p) == 1
    p.close()
    assert state['finalised'] and state['made'] < 1000


def test_timed_accumulates_under_its_key():
    L.LOADER_TIMES.pop('a_test_key', None)
    for _ in range(2):
        with L.timed('a_test_key'):
            pass
    assert L.LOADER_TIMES.pop('a_test_key') >= 0.0
    from vitcap_amd import pipeline as P
    assert P.LOADER_TIMES is L.LOADER_TIMES and isinstance(P.LAST_PREDICT_STATS, dict)
