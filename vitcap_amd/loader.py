"""Test-set loader: one rank's rows of a (key, base64 JPEG) TSV -> batches {'image', 'key'} for
CaptionUniPipeline.predict.  Rank r takes rows r, r+world, ... like DistributedSampler(shuffle=False) (uni_pipeline.py:782-850); the
images are decoded on the host by a pool of workers (jpegdec.py) and transformed on the GPU (csrc/preproc.hip).  The pieces:

* decode_ahead_plan  how many batches are decoded ahead and how many shared-memory slabs that takes;
* decode_executor    the worker pool: spawned processes, pinned processes or threads;
* SlabPool           the page-locked shared-memory slabs the workers decode into, and the rule for their reuse;
* PredictBatchLoader submits decode tasks `ahead` batches ahead and assembles the batches in order;
* prefetched         runs any batch generator on a background thread with a stream of its own;
* LOADER_TIMES / timed   where the producer thread and the consumer waited.

The task functions themselves live in jpegdec.py: a spawned worker imports that module only, never this one or torch."""
import collections
import contextlib
import logging
import os
import time

import numpy as np
import torch

from .jpegdec import coef_item, decode_rows, decode_rows_into

LOADER_TIMES = {}           # seconds, summed over the batches of the last predict: where the producer thread and the consumer waited


@contextlib.contextmanager
def timed(key):
    """Adds the seconds spent inside the block to LOADER_TIMES[key]."""
    t0 = time.perf_counter()
    yield
    LOADER_TIMES[key] = LOADER_TIMES.get(key, 0.0) + time.perf_counter() - t0


Plan = collections.namedtuple('Plan', 'per_batch ahead n_slabs')


def decode_ahead_plan(bs, workers, chunk, slab_bytes, budget, use_slabs, ahead_override=None):
    """-> Plan(worker tasks per batch, batches decoded ahead of the one handed out, shared-memory slabs).  `chunk` images per worker
    task; `ahead_override` is VITCAP_LOADER_AHEAD when set; without slabs (threads, pipe return) n_slabs is 0."""
    per_batch = (bs + chunk - 1) // chunk
    # batches being decoded ahead of the one handed out: ten tasks per worker.  Decode times jitter (image sizes, a host shared
    # with other tenants) and the consumer can never run faster than the GPU to make up for a gap, so every gap is lost for good:
    # with 3 batches ahead + 4 queued 0.93-0.94 of the resident rate, with 10 + 24 0.96-0.975 (profiles/r05_input_side.json)
    ahead = min(12, max(3, (10 * workers + per_batch - 1) // per_batch))     # <= 15 batches of slabs (2.9 GB nominal) however many workers
    if ahead_override is not None:
        ahead = int(ahead_override)
    if not use_slabs:
        return Plan(per_batch, ahead, 0)
    # the slabs are page-locked shared memory (x ranks on one host): the decode-ahead depth is capped in BYTES, not batches
    # (at test_batch_size 512 the batch-count rule asked for 9-23 GB per rank).  The floor is one batch ahead + the
    # three in retirement.
    ahead = max(1, min(ahead, budget // (per_batch * slab_bytes) - 3))
    return Plan(per_batch, ahead, (ahead + 3) * per_batch)


def decode_executor(workers, threads=False, cpus=None):
    """JPEG decoding is host work: `workers` worker PROCESSES (the reference's DataLoader(num_workers), uni_pipeline.py:333-339)
    decode the images of the next batches while the GPU captions the current one.  Measured on the GPU box
    (tools/input_side_bench.py, profiles/r04_input_side.json): one core decodes 600 images/s, threads of one process top out near
    2 000 (GIL), a GPU captions 3 700.  The workers are SPAWNED (never forked: this process owns a GPU context) and import
    vitcap_amd.jpegdec only.  `threads` (`loader_threads: true`) keeps the decode in threads of this process.
    `cpus` = VITCAP_LOADER_CPUS=<first>[:<stride>] (experiment): worker i is pinned to CPU first + i * stride (default stride 1) --
    under a CFS quota on a many-core host the scheduler otherwise migrates the decoders across the whole machine."""
    from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
    if threads:
        return ThreadPoolExecutor(max_workers=workers)
    import multiprocessing as mp
    ctx = mp.get_context('spawn')
    if not cpus:
        return ProcessPoolExecutor(max_workers=workers, mp_context=ctx)
    from .jpegdec import pin_worker
    first, _, stride = cpus.partition(':')
    return ProcessPoolExecutor(max_workers=workers, mp_context=ctx, initializer=pin_worker,
                               initargs=(ctx.Value('i', 0), int(first), int(stride or 1)))


def _release_slab(shm):
    """close() raises BufferError while a numpy view of the segment is still exported; the name must be unlinked all the same, or the
    segment outlives the process until the resource tracker reaps it."""
    try:
        shm.close()
    except Exception:
        pass
    try:
        shm.unlink()
    except Exception:
        pass


def _pin_slabs(slabs):
    """hipHostRegister on every shared-memory slab -> list of registered base addresses (empty when the runtime refuses: the copies
    then take the pageable path, slower but correct).  VITCAP_LOADER_PIN=0 disables."""
    import ctypes
    if os.environ.get('VITCAP_LOADER_PIN', '1') == '0':
        return []
    done = []
    try:
        rt = torch.cuda.cudart()
        for shm in slabs:
            addr = ctypes.addressof(ctypes.c_char.from_buffer(shm.buf))
            err = rt.cudaHostRegister(addr, shm.size, 0)
            if int(getattr(err, 'value', err)) != 0:
                logging.warning('hipHostRegister refused a loader slab (error %s): host -> device copies stay pageable', err)
                break
            done.append(addr)
    except Exception as e:          # noqa
        logging.warning('loader slabs not page-locked (%s)', e)
    return done


def _unpin_slabs(addrs):
    try:
        rt = torch.cuda.cudart()
        for a in addrs:
            rt.cudaHostUnregister(a)
    except Exception:
        pass


class SlabPool(object):
    """The shared-memory slabs of a plan.  Decoded pixels come back through shared memory (jpegdec.py); a slab holds one task's images
    and is reused two batches after the batch that read it went to the GPU: take() hands a free slab to a new task, retire(ids) takes
    the slabs of the batch just handed out and frees those of the second batch before it.  An empty pool (plan.n_slabs == 0, or
    no room) is false: the images then return through the executor's own channel.
    `device`: the stream whose copies read the slabs is synchronised before they are released (None: nothing to wait for)."""

    def __init__(self, plan, slab_bytes, device=None):
        from multiprocessing import shared_memory
        self.device, self.segments, self.pinned, self.retired = device, [], [], []
        if plan.n_slabs:
            logging.info('loader: %d slabs x %d MB = %.1f GB of page-locked shared memory (%d batches ahead)', plan.n_slabs, slab_bytes >> 20,
                         plan.n_slabs * slab_bytes / 2**30, plan.ahead)
        # a /dev/shm too small for the slabs (container default: 64 MB) would kill the workers with SIGBUS on first touch:
        # check the free space first and fall back to returning the pixels through the pool's pipe (decode_rows)
        try:
            st = os.statvfs('/dev/shm')
            room = st.f_bavail * st.f_frsize
        except OSError:
            room = 0
        if room >= (plan.n_slabs * slab_bytes * 5) // 4:
            try:
                for _ in range(plan.n_slabs):
                    self.segments.append(shared_memory.SharedMemory(create=True, size=slab_bytes))
            except OSError as e:
                logging.warning('shared-memory slabs unavailable (%s): decoded images return through the worker pipe', e)
                self._release()
        else:
            logging.warning('/dev/shm has %.0f MB free, the loader wants %.0f MB of slabs: decoded images return through the worker '
                            'pipe (lower num_workers / loader_slab_mb, or enlarge /dev/shm)', room / 2**20, plan.n_slabs * slab_bytes / 2**20)
        self.free = list(range(len(self.segments)))
        # page-lock the slabs: a pageable source makes every host -> device copy go through the runtime's staging buffer (a
        # single-threaded memcpy of ~1 MB per image in THIS process, then the DMA); registered, the DMA reads the slab itself
        if self.segments:
            self.pinned = _pin_slabs(self.segments)

    def __len__(self):
        return len(self.segments)

    def take(self):
        return self.free.pop()

    def retire(self, ids):
        self.retired.append(ids)                    # slab ids of the last batches handed to the GPU
        if len(self.retired) > 2:
            self.free.extend(self.retired.pop(0))

    def _release(self):
        for shm in self.segments:
            _release_slab(shm)
        self.segments = []

    def close(self):
        if self.segments and self.device is not None:
            try:
                torch.cuda.current_stream(self.device).synchronize()     # no copy still reads a slab
            except Exception:
                pass
        if self.pinned:
            _unpin_slabs(self.pinned)
        self._release()
        self.pinned, self.free, self.retired = [], [], []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class PredictBatchLoader(object):
    """Iterator over the batches {'image': preprocess(images), 'key': [...]} of the rows `row_ids` of the TSV file `tsv`, `bs` rows per
    batch, in row order.  Rows are read by the WORKERS: a task names the file and up to `chunk` row numbers (jpegdec.decode_rows_into
    with a slab, jpegdec.decode_rows without); `plan.ahead` batches are being decoded while one is assembled.  The loader owns
    `executor` and `slabs`: exhaustion, close() and an exception (a worker's included) shut the executor down -- waiting for the tasks
    still writing into slabs -- and then release the slabs."""

    def __init__(self, tsv, row_ids, bs, chunk, plan, executor, slabs, device_jpeg, preprocess):
        self.tsv, self.row_ids, self.bs, self.chunk, self.ahead = tsv, row_ids, bs, chunk, plan.ahead
        self.executor, self.slabs, self.device_jpeg, self.pre = executor, slabs, device_jpeg, preprocess
        self._batches = self._run()

    def __iter__(self):
        return self

    def __next__(self):
        return next(self._batches)

    def close(self):
        self._batches.close()
        self.executor.shutdown()        # both are no-ops after _run's own exit; they matter when it never started
        self.slabs.close()

    def _submit(self, ids):
        """One batch's tasks -> [(slab id or None, future)]."""
        tasks = []
        for c in range(0, len(ids), self.chunk):
            if self.slabs:
                sid = self.slabs.take()
                tasks.append((sid, self.executor.submit(decode_rows_into, self.slabs.segments[sid].name, self.tsv, ids[c:c + self.chunk],
                                                        self.device_jpeg)))
            else:
                tasks.append((None, self.executor.submit(decode_rows, self.tsv, ids[c:c + self.chunk])))
        return tasks

    def _collect(self, tasks):
        """Waits for one batch's tasks in order -> (keys, images, slab ids used)."""
        from .imageio import CoefImage          # loads the HIP library: not at import time, the pipeline module imports this one
        keys, imgs, used = [], [], []
        for sid, f in tasks:
            ks, items = f.result()
            keys.extend(ks)
            buf = self.slabs.segments[sid].buf if sid is not None else None
            for item in items:
                if sid is not None and isinstance(item, tuple) and item[0] == 'coef':
                    imgs.append(CoefImage(*coef_item(item, buf)))     # the GPU finishes the decode (csrc/jpeg.hip)
                elif sid is not None and isinstance(item, tuple):
                    off, h, w = item
                    imgs.append(np.ndarray((h, w, 3), dtype=np.uint8, buffer=buf, offset=off))
                else:
                    imgs.append(item)       # an array through the pipe: no slabs, or an image that did not fit its slab
            if sid is not None:
                used.append(sid)
        return keys, imgs, used

    def _run(self):
        todo = [self.row_ids[s:s + self.bs] for s in range(0, len(self.row_ids), self.bs)]
        with self.slabs, self.executor:         # left in reverse: the workers are done before their slabs go
            inflight = [self._submit(todo.pop(0)) for _ in range(min(self.ahead, len(todo)))]
            while inflight:
                with timed('decode_wait'):
                    keys, imgs, used = self._collect(inflight.pop(0))
                with timed('transform_enqueue'):
                    batch = {'image': self.pre(imgs), 'key': keys}       # host -> device copies of pageable memory return once staged
                    del imgs
                self.slabs.retire(used)
                if todo:
                    inflight.append(self._submit(todo.pop(0)))
                yield batch


def prefetched(gen, device, depth=2):
    """Runs the batch generator in a background thread, `depth` batches ahead: reading the TSV rows, handing them to the decode workers,
    the host -> device copies and the launch of the transform kernel no longer sit between two caption launches of the consumer
    (measured: the consumer thread was the limit at 26 ms per batch of 64, the GPU needs 17).  A batch is handed over after the producer's
    stream has been synchronised, so the consumer may use it on any stream."""
    import queue
    import threading
    q = queue.Queue(maxsize=max(1, depth))
    END = object()
    stop = threading.Event()            # set when the consumer goes away (exception, generator closed): the producer must not block in put

    def put(item):
        while not stop.is_set():
            try:
                q.put(item, timeout=0.2)
                return True
            except queue.Full:
                continue
        return False

    def work():
        try:
            if device.type == 'cuda':
                torch.cuda.set_device(device)
            ev = torch.cuda.Event(blocking=True) if device.type == 'cuda' else None     # sleep, do not spin (see generate_async)
            # the producer's copies and transform kernels go to a stream of their own: on the (per-process) default stream they shared a
            # queue with the consumer's blocking device -> host copies of the finished captions, and each side waited behind the other's
            # work -- with 24 batches of prefetch a `.cpu()` of 5 KB could sit behind a whole batch of host -> device copies
            # (docs/LAB_r05.md 5: the 22 ms-per-batch mode of the round script's input-side runs)
            if device.type == 'cuda':
                from .model import role_stream
                torch.cuda.set_stream(role_stream(device, 'loader', lambda: torch.cuda.Stream(device)))     # thread-local: this thread only
            for b in gen:
                with timed('copy_sync'):
                    if ev is not None:
                        ev.record(torch.cuda.current_stream(device))
                        ev.synchronize()
                with timed('queue_full'):
                    ok = put(b)
                if not ok:
                    break
            else:
                put(END)
        except BaseException as e:          # surfaces in the consumer
            put(e)
        finally:
            close = getattr(gen, 'close', None)     # runs the generator's own `finally` (worker pool, shared-memory slabs) in this thread
            if close is not None:
                try:
                    close()
                except Exception:
                    pass
    t = threading.Thread(target=work, daemon=True)
    t.start()
    try:
        while True:
            with timed('queue_empty'):
                b = q.get()
            if b is END:
                break
            if isinstance(b, BaseException):
                raise b
            yield b
    finally:
        stop.set()
        t.join(timeout=30)
