"""Device engine: thin, typed Python wrapper around one ``cna_ctx`` of libcna_hip.so.

One Engine per process/GPU.  It owns the device-resident graph, diffusion state, NAM and
working matrix; the host code in ``cna_amd.tools`` drives it step by step the way the
reference drives numpy/scipy.  Nothing here computes on the CPU.
"""
import ctypes as C
import os
import weakref

import numpy as np
import scipy.sparse as sp

from . import _ffi, _order
from ._ffi import check, ptr, MAT_NAM, MAT_X

# the integer results (s_lo, s_hi) one cna_gene_rank_corr_x_by call may return: Engine.gene_rank_corr_x_by takes its columns in
# chunks within it.  The figure of Engine.CROSS_BY_HOST_BYTES; a module constant so that a test can lower it
RANK_X_BY_HOST_BYTES = 1 << 30


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def array_digest(a):
    """128-bit content hash of an array's bytes, as hex."""
    import hashlib
    return hashlib.blake2b(np.ascontiguousarray(a).view(np.uint8).reshape(-1), digest_size=16).hexdigest()


def _rows_of_x(xrow, n_rows, codes, W=None):
    """Caller-order `codes` (int32 per cell) and the columns of `W` (q x cells, or None) scattered onto the n_rows rows of
    X: cell i goes to row xrow[i]; a cell without a row is left out, a row without a cell gets code -1 and weight 0."""
    has = np.flatnonzero((xrow >= 0) & (xrow < n_rows))
    local = np.full(n_rows, -1, dtype=np.int32)
    local[xrow[has]] = codes[has]
    if W is None:
        return local, None
    Wl = np.zeros((W.shape[0], n_rows))
    Wl[:, xrow[has]] = W[:, has]
    return local, Wl


class _Memo:
    """What expr_cross / expr_cross_by keep of their last launch: `key` = _x_key then, `content` the caller's word for what
    X was made from, `tag` what else a hit needs equal (expr_cross_by: the codes' digest and n_bins), `result`, and `extra`,
    a dict for what else a caller derives from the same inputs."""
    __slots__ = ('key', 'content', 'tag', 'result', 'extra')

    def __init__(self, key, content, tag, result):
        self.key, self.content, self.tag, self.result, self.extra = key, content, tag, result, {}


def _x_key(engine, info):
    """(uploads of the expression matrix `info` describes, or None without one; x_epoch; the library's X generation)"""
    return (info['uploads'] if info['format'] != 'none' else None, engine.x_epoch, engine.x_generation())


def _memo_lookup(memo, key, content, tag):
    """`memo` when it serves a call under (key, content, tag), else None.  An equal key and tag: a hit, whatever the content.
    A moved key: a hit only under the same upload, an equal tag and an equal content that is not None -- the entry is carried
    over, re-keyed, its extra with it."""
    if memo is None or key[0] is None or memo.tag != tag:
        return None
    if memo.key != key:
        if content is None or memo.content != content or memo.key[0] != key[0]:
            return None
        memo.key = key
    return memo


def _memo_store(key, content, tag, result):
    """A fresh entry (empty extra) for `result`, whose arrays become read-only."""
    for a in result:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return _Memo(key, content, tag, result)


class Engine(_order.CellOrder):
    def __init__(self, device=None, rank=0, nranks=1, unique_id=None, shm=None):
        """unique_id: RCCL id from rank 0 (one GPU per rank).  shm: (segment name, slot bytes) selects
        the host-staged test communicator instead, which lets several ranks share one GPU."""
        self.lib = _ffi.load()
        if device is None:
            device = int(os.environ.get('LOCAL_RANK', '0')) if nranks > 1 else 0
        h = _ffi.c_ctx()
        check(self.lib.cna_ctx_create(int(device), C.byref(h)), 'cna_ctx_create')
        self.h = h
        self.device = int(device)
        self.rank, self.nranks = int(rank), int(nranks)
        if nranks > 1 and unique_id is None and shm is None:
            raise ValueError('nranks > 1 needs the RCCL unique id created by rank 0')
        self._has_comm = unique_id is not None or shm is not None
        self.halo_comm = False
        if shm is not None:
            check(self.lib.cna_comm_init_shm(self.h, self.rank, self.nranks, str(shm[0]).encode(), int(shm[1])),
                  'cna_comm_init_shm')
        elif unique_id is not None:   # also with one rank: every collective then really goes through RCCL
            buf = (C.c_char * 128).from_buffer_copy(bytes(unique_id))
            check(self.lib.cna_comm_init(self.h, self.rank, self.nranks, C.cast(buf, C.c_void_p)), 'cna_comm_init')
            # a rank that cannot reach a peer should say so now, not hang in the first collective of an analysis
            ok = C.c_int(0)
            check(self.lib.cna_comm_selftest(self.h, float(os.environ.get('CNA_COMM_TIMEOUT', '120')), C.byref(ok)),
                  'cna_comm_selftest')
            self.halo_comm = bool(ok.value)     # the halo exchange has a communicator of its own (overlaps the walk step)
        self._graph_key = None
        self._graph_hash = None
        self._pending_check = None
        self._defer_graph_check = False
        self._graph_ref = None
        self._pinned = None
        self._expr_key = self._expr_hash = self._expr_ref = self._expr_pinned = None
        self._cross_memo = None     # the _Memo of the last expr_cross; None voids it
        self.cross_launches = 0     # cna_expr_cross calls so far (a memo hit launches nothing)
        self._cross_by_memo = None  # the _Memo of the last expr_cross_by, its tag (codes digest, n_bins); None voids it
        self.cross_by_launches = 0  # expr_cross_by calls that went to the device (a memo hit launches nothing)
        self._host_threads = _order.usable_cpus(8)
        self._colsum_w = None
        self._codes_token = self._codes_graph = None
        self._assoc_out = None
        self._zc_cols = 0
        self._fused = None
        self.n = 0            # cells in the caller's view: all of them, or (view_local) this rank's block
        self.n_global = 0
        self.row0 = 0
        self.n_local = 0
        self.N = 0
        self.x_rows_total = 0
        self.x_epoch = 0      # bumped whenever the working matrix X is replaced
        self.nam_epoch = 0    # bumped whenever a new NAM is started
        # keep the NAM across analyses of one dataset (tools._nam._nam_device); engine.reuse_nam = False recomputes it
        # every call (what bench.py measures)
        self.reuse_nam = True
        # ... and, opt-in, the standardised NAM of an analysis without covariates and batches: a further phenotype then
        # only takes new coefficients (tools._association.compute_nam_and_reindex)
        self.reuse_x = False

    # ---------------------------------------------------------------- lifetime
    def close(self):
        if getattr(self, 'h', None):
            self.lib.cna_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def comm_info(self):
        """(backend, nranks) of the communicator: 'none' | 'rccl' | 'shm', and the rank count it reports."""
        b, n = C.c_int(0), C.c_int(0)
        check(self.lib.cna_comm_info(self.h, C.byref(b), C.byref(n)), 'cna_comm_info')
        return ('none', 'rccl', 'shm')[b.value], n.value

    def sync(self):
        check(self.lib.cna_ctx_sync(self.h), 'cna_ctx_sync')

    def set_state_f32(self, on=True):
        """Opt-in: keep the diffusion state between two steps of a walk in 4 bytes per entry (one rank, more than 64
        samples; sums, NAM and everything downstream stay float64).  Halves what the dense step gathers; the NAM then
        agrees with the default walk to ~1e-7 relative instead of bit for bit (reference: float64 `s` between the
        iterations of `_nam.py:31-34`).  A NAM held on the device from the other format is forgotten."""
        on = bool(on)
        if on != getattr(self, '_state_f32', None):
            check(self.lib.cna_set_state_f32(self.h, int(on)), 'cna_set_state_f32')
            self._state_f32 = on
            self._nam_sig = None
        return self

    def device_bytes(self):
        b = C.c_int64(0)
        check(self.lib.cna_ctx_device_bytes(self.h, C.byref(b)), 'cna_ctx_device_bytes')
        return b.value

    @staticmethod
    def new_unique_id():
        lib = _ffi.load()
        buf = (C.c_char * 128)()
        check(lib.cna_comm_unique_id(C.cast(buf, C.c_void_p)), 'cna_comm_unique_id')
        return bytes(buf)

    # ---------------------------------------------------------------- graph
    def block(self, n):
        """Rows [r0, r1) of an n-cell problem owned by this rank (ceil split)."""
        rpr = -(-n // self.nranks)
        r0 = min(self.rank * rpr, n)
        return r0, min(r0 + rpr, n)

    def _quick_key(self, A):
        """Cheap identity of a graph: the scipy object, its buffers, sizes and dtypes, and a hash of three
        64 KB windows (head, middle, tail) of values and indices (~20 us).  Necessary, not sufficient."""
        ident = self._ident(A)
        w = 16384
        mid = max(0, A.nnz // 2 - w // 2)
        parts = [slice(0, w), slice(mid, mid + w), slice(max(0, A.nnz - w), A.nnz)]
        probe = tuple(self._hash(arr[p_], 1) for arr in (A.data, A.indices) for p_ in parts)
        return ident + probe

    def _ident(self, A):
        return (A.shape, int(A.nnz), str(A.data.dtype), str(A.indices.dtype), str(A.indptr.dtype), id(A)) + self._buffers(A)

    def _full_hash(self, A):
        """64-bit hashes of the FULL content of data, indices and indptr (csrc/host_graph.c, several
        threads: ~0.5 ms for the 66 MB of a 200k-cell graph, 4.6 ms at 2M cells) -- an in-place edit of
        any entry changes it, and the graph then goes to the device again, as the reference re-reads the
        matrix on every call (_nam.py:25-28)."""
        return tuple(self._hash(arr) for arr in (A.data, A.indices, A.indptr))

    @staticmethod
    def _buffers(A):
        return (A.data.ctypes.data, A.indices.ctypes.data, A.indptr.ctypes.data)

    def _hash(self, arr, threads=None):
        arr = np.ascontiguousarray(arr)
        return int(self.lib.cna_host_hash64(ptr(arr), arr.nbytes, self._host_threads if threads is None else threads))

    def graph_resident(self, A):
        """Cheap and conservative: True when A is, by object and buffers, the matrix whose copy is on the device (whether
        its content still is what went up is ensure_graph's business)."""
        try:
            return (self._graph_key is not None and self._graph_ref is not None and self._graph_ref() is A
                    and self._graph_key[:len(self._ident(A))] == self._ident(A))
        except Exception:                      # noqa: BLE001
            return False

    def pin_graph(self, A):
        """Promise that the connectivities matrix A will not be edited in place while it is resident:
        later calls then recognise it without hashing all of it (what a loop over many phenotypes of
        one dataset wants; bench.py does this and says so).  `unpin_graph()` withdraws the promise."""
        if not sp.isspmatrix_csr(A) and not isinstance(A, sp.csr_array):
            raise TypeError('pin_graph needs the CSR matrix that is passed to the analysis')
        self._pinned = (weakref.ref(A), self._buffers(A))

    def unpin_graph(self):
        self._pinned = None

    # ---- the device cell order of a large graph, computed beside its first analyses
    def _start_reorder(self, A):
        self._drop_reorder()
        box = {'ref': weakref.ref(A), 'buffers': self._buffers(A), 'ident': self._ident(A)}

        def job():
            perm = _order.locality_order(A)
            if perm is None:
                return None
            # (the content the order was made from: adopted only if the matrix still hashes to it.  The renumbered rows
            # themselves are made on the device from the resident copy: cna_graph_reorder)
            return np.ascontiguousarray(perm, dtype=np.int64), self._full_hash(A)
        box['future'] = _reorder_pool().submit(job)
        self._reorder = box

    def _drop_reorder(self):
        self._reorder = None

    def _take_reorder(self, A):
        """The finished order for this very matrix (same object, same buffers), else None; never waits."""
        box = getattr(self, '_reorder', None)
        if box is None or box['ref']() is not A or box['buffers'] != self._buffers(A) or not box['future'].done():
            return None
        self._reorder = None
        try:
            out = box['future'].result()
        except Exception:                      # noqa: BLE001 - the caller's order stays
            return None
        if out is None or out[1] != self._graph_hash:
            return None                        # edited in place since: the next content check uploads it afresh
        pinned = self._pinned is not None and self._pinned[0]() is A and self._pinned[1] == self._buffers(A)
        if not pinned and self._full_hash(A) != out[1]:
            return None                        # ... or edited after the order was made (an unpinned matrix is hashed in full, as always)
        return out

    def reorder_pending(self):
        """True while the cell order of the resident graph is still being computed beside the analyses (the
        graph is then resident in the caller's order: same results, a slower random walk)."""
        box = getattr(self, '_reorder', None)
        return box is not None

    def wait_reorder(self):
        """Block until that computation has finished (benchmarks: the next call adopts it)."""
        box = getattr(self, '_reorder', None)
        if box is not None:
            try:
                box['future'].result()
            except Exception:                  # noqa: BLE001
                pass

    def ensure_graph(self, A, shard=None, defer=False):
        """Upload the connectivities graph unless this very matrix -- same object, same content -- is
        already resident.  The cells are kept on the device in a locality-preserving order (see
        _order.py); everything that crosses this class's boundary is in the caller's order.

        Content check: the full hash of data / indices / indptr (`_full_hash`), unless the matrix is
        pinned (`pin_graph`).  defer=True (one GPU only): when the cheap identity matches, return at once
        and take the full hash on a helper thread; the caller MUST call `confirm_graph()` before it lets
        any result out and start over if that returns False (tools._association does).

        shard=None: A is the whole n x n graph (on every rank; each keeps its row block).
        shard=(row0, n_global): A holds only the rows [row0, row0 + A.shape[0]) of the graph, with
        global column ids -- the block engine.block(n_global) assigns to this rank.  The engine then
        works in the local view: every per-cell input and output covers this rank's cells only."""
        if not sp.issparse(A):
            raise TypeError('connectivities must be a scipy.sparse matrix')
        if not sp.isspmatrix_csr(A) and not isinstance(A, sp.csr_array):
            A = sp.csr_matrix(A)
        if shard is None and A.shape[0] != A.shape[1]:
            raise ValueError('connectivities must be square')
        self._pending_check = None
        pinned = self._pinned is not None and self._pinned[0]() is A and self._pinned[1] == self._buffers(A)
        shard_key = None if shard is None else tuple(int(v) for v in shard)
        staged = None
        if pinned and self._graph_key is not None and self._graph_ref is not None and self._graph_ref() is A:
            # pinned: the caller's promise replaces the content probes (six 64 KB windows from cold memory: 0.15 ms)
            ident = self._ident(A)
            if self._graph_key[:len(ident)] == ident and self._graph_key[-1] == shard_key:
                staged = self._take_reorder(A)
                if staged is None:
                    return False
        if (staged is None and defer == 'caller' and not pinned and self.nranks == 1 and not self._has_comm
                and self._graph_key is not None and self._graph_ref is not None and self._graph_ref() is A
                and getattr(self, '_reorder', None) is None):
            # the caller has ALL of the matrix hashed while the device works (take_pending_graph: inside
            # cna_assoc_finish): the probes of the quick key (six 64 KB windows: 0.1 ms) would tell it nothing more
            ident = self._ident(A)
            if self._graph_key[:len(ident)] == ident and self._graph_key[-1] == shard_key:
                self._pending_check = ('caller', A)
                return False
        quick = self._quick_key(A) + (shard_key,)
        full = None
        if staged is None and self._graph_key == quick and self._graph_ref is not None and self._graph_ref() is A:
            staged = self._take_reorder(A)
            if staged is not None:
                pass
            elif pinned:
                return False
            elif defer == 'caller' and self.nranks == 1 and not self._has_comm:
                # the caller has the three arrays hashed itself (take_pending_graph: inside cna_assoc_finish, while the
                # device works); confirm_graph() still settles it if the caller never takes it
                self._pending_check = ('caller', A)
                return False
            elif defer and self.nranks == 1 and not self._has_comm:
                self._pending_check = _checker().submit(self._full_hash, A)
                return False
            else:
                full = self._full_hash(A)
                if full == self._graph_hash:
                    return False
        if staged is None:
            self._drop_reorder()
        key = quick
        if staged is not None:
            # the device cell order computed beside the first analyses of this graph (see below) has arrived: the
            # resident copy is renumbered ON THE DEVICE (the rows keep the order of their entries: same bits as an upload
            # of the renumbered graph, without the second trip over PCIe); column sums and sample codes move with it,
            # everything else per cell follows as after any upload
            perm, full = staged
            try:
                check(self.lib.cna_graph_reorder(self.h, ptr(perm)), 'cna_graph_reorder')
            except _ffi.CnaHipError:
                # the device order is an optimisation (a second copy of the graph plus temporaries: it can run out of
                # memory); the library leaves the resident copy in the caller's order intact -- that order stays
                return False
            self.perm = perm
            self._keep_dev = None
            self._kept_order_cache = None
            self._x_is_selection = False
            self._graph_key = key
            self._graph_hash = full
            self._pending_check = None
            return True
        elif shard is None:
            n = A.shape[0]
            r0, r1 = self.block(n)
            # A large graph that is new to the device goes up in the caller's order first: the cluster order takes
            # longer than the analysis (0.3 s against 0.02 s at 2M cells) and results do not depend on the device order
            # -- so it is computed on a host thread meanwhile and adopted by the first later call that finds it done
            # (CNA_REORDER_ASYNC=0: in line, as before)
            lazy = (self.nranks == 1 and not self._has_comm and n >= _REORDER_ASYNC_CELLS and _REORDER_ASYNC
                    and os.environ.get('CNA_REORDER', '1') not in ('0', 'off', 'no'))
            perm = None if lazy else _order.locality_order(A)
            if lazy:
                self._start_reorder(A)
            if perm is None:
                lo, hi = int(A.indptr[r0]), int(A.indptr[r1])
                indptr = np.ascontiguousarray(A.indptr[r0:r1 + 1].astype(np.int64) - lo)
                indices = np.ascontiguousarray(A.indices[lo:hi], dtype=np.int32)
                data = A.data[lo:hi]
            else:
                indptr, indices, data = _order.permuted_rows(A, perm, r0, r1)
            order = None if perm is None else perm[r0:r1]
        else:
            r0, n = int(shard[0]), int(shard[1])
            r1 = r0 + A.shape[0]
            if A.shape[1] != n or (r0, r1) != self.block(n):
                raise ValueError('rank %d of %d owns rows [%d, %d) of %d cells (engine.block); got rows [%d, %d) '
                                 'of a %d-column graph' % ((self.rank, self.nranks) + self.block(n) + (n, r0, r1, A.shape[1])))
            # locality order inside the block (RCM of its diagonal part); the ranks exchange their
            # orders once, so that each can relabel the columns that point into other blocks
            perm = _order.locality_order(A[:, r0:r1]) if r1 > r0 else None
            if perm is None:
                perm = np.arange(r1 - r0, dtype=np.int64)
            col_map = _order.inverse(self._allgather_i64(perm + r0))
            indptr, indices, data = _order.permuted_rows(A, perm, 0, r1 - r0, col_map=col_map)
            order = perm
        if data.dtype == np.float32:
            data, f64 = np.ascontiguousarray(data), 0
        else:
            data, f64 = np.ascontiguousarray(data, dtype=np.float64), 1
        check(self.lib.cna_set_local_view(self.h, int(shard is not None)), 'cna_set_local_view')
        check(self.lib.cna_graph_upload(self.h, n, r0, r1 - r0, ptr(indptr), ptr(indices), ptr(data), f64),
              'cna_graph_upload')
        if order is not None:
            check(self.lib.cna_set_cell_order(self.h, ptr(np.ascontiguousarray(order))), 'cna_set_cell_order')
        self.halo = None
        if self.nranks > 1 or (self._has_comm and os.environ.get('CNA_HALO_SELFTEST')):
            plan = _order.halo_plan(indices, r0, r1 - r0, -(-n // self.nranks), self.rank, self.nranks,
                                    self._allgather_i64,
                                    force_self=int(os.environ.get('CNA_HALO_SELFTEST', '0')))
            if plan is not None and os.environ.get('CNA_HALO', '1') not in ('0', 'off'):
                send_rows, send_counts, recv_rows, recv_counts = plan
                check(self.lib.cna_set_halo(self.h, ptr(send_rows), ptr(send_counts), ptr(recv_rows),
                                            ptr(recv_counts)), 'cna_set_halo')
                self.halo = (int(send_counts.sum()), int(recv_counts.sum()))
        self.perm = perm
        self.view_local = shard is not None
        self._keep_dev = None
        self._kept_order_cache = None
        self._x_is_selection = False
        self.n_global, self.row0, self.n_local = n, r0, r1 - r0
        self.n = self.n_local if self.view_local else n
        self._graph_key = key
        self._graph_hash = full if full is not None else self._full_hash(A)
        self._pending_check = None
        try:
            self._graph_ref = weakref.ref(A)
        except TypeError:
            self._graph_ref = None
        self._colsum_w = None
        self._codes_token = self._codes_graph = None
        return True

    def confirm_graph(self):
        """Outcome of the deferred content check of ensure_graph(defer=True): True = the resident graph is
        the caller's graph (or nothing was deferred).  False: the matrix was edited in place since it went
        to the device; the resident copy is dropped and the caller has to redo its work."""
        fut, self._pending_check = self._pending_check, None
        if fut is None:
            return True
        if isinstance(fut, tuple):
            if self._full_hash(fut[1]) == self._graph_hash:
                return True
        elif fut.result() == self._graph_hash:
            return True
        self.drop_graph()
        return False

    def take_pending_graph(self):
        """The deferred check of ensure_graph(defer='caller') as [(array, 64-bit hash its content must have)] x 3 for a
        caller that has them verified elsewhere (and calls drop_graph() when that fails); else None."""
        fut = self._pending_check
        if not isinstance(fut, tuple) or self._graph_hash is None:
            return None
        self._pending_check = None
        A = fut[1]
        return [(np.ascontiguousarray(arr), h) for arr, h in zip((A.data, A.indices, A.indptr), self._graph_hash)]

    def drop_graph(self):
        """Forget the resident graph (its content is no longer what the caller holds): the next call uploads afresh."""
        self._graph_key = None
        self._graph_hash = None
        self._nam_sig = None

    def colsums(self, self_weight=1):
        w = float(self_weight)
        if self._colsum_w != w:
            check(self.lib.cna_colsums(self.h, w), 'cna_colsums')
            self._colsum_w = w

    def fetch_colsums(self):
        out = np.empty(self.n_global)
        check(self.lib.cna_fetch_colsums(self.h, ptr(out)), 'cna_fetch_colsums')
        return self.cells_to_user(out[self.row0:self.row0 + self.n_local] if self.view_local else out)

    # ---------------------------------------------------------------- NAM
    def set_samples(self, codes, n_samples, counts, token=None):
        """Sample code per cell + cells per sample.  ``token``: an opaque, hashable identity of
        `codes` (see tools._nam.sample_codes_cached); when it equals the token of the codes already
        on the device for this graph, the upload is skipped and only the walk is restarted."""
        if token is not None and token == self._codes_token and self._codes_graph == self._graph_key:
            check(self.lib.cna_restart_nam(self.h), 'cna_restart_nam')
            self.nam_epoch += 1
            return
        if len(codes) != self.n:
            raise ValueError('need one sample code per cell')
        codes = self.cells_to_device(np.asarray(codes))
        if self.view_local:      # every rank needs the sample of every cell (first walk step): blocks in rank order
            codes = self._allgather_i64(codes)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        counts = _f64(counts)
        check(self.lib.cna_set_samples(self.h, ptr(codes), int(n_samples), ptr(counts)), 'cna_set_samples')
        self.N = int(n_samples)
        self.nam_epoch += 1
        self._codes_token, self._codes_graph = token, self._graph_key

    def nam_step(self, want_kurt, may_continue, may_stop):
        check(self.lib.cna_nam_step(self.h, int(bool(want_kurt)), int(bool(may_continue)), int(bool(may_stop))),
              'cna_nam_step')

    def nam_steps(self, nsteps):
        """nsteps walk steps in one call (fixed step count, nothing for the host to decide in between)."""
        check(self.lib.cna_nam_steps(self.h, int(nsteps)), 'cna_nam_steps')

    def nam_select_hint(self, y_std):
        """Tell the walk in progress which standardised phenotype select_standardized() will be called with (all
        cells, samples in place, nothing regressed out): its last step then does that pass on its way out."""
        yv = None if y_std is None else _f64(y_std)
        check(self.lib.cna_nam_select_hint(self.h, ptr(yv), 0 if yv is None else len(yv)), 'cna_nam_select_hint')
        if yv is not None:
            # the step that follows overwrites the working matrix: results of earlier calls that still read it lazily
            # (res.namresid, res.namresid_nbhdXpc) must see that now, not only once select_standardized() has run
            self.x_epoch += 1

    def nam_auto(self, maxnsteps=15):
        """The walk with the reference's stop rule (nsteps=None, _nam.py:64-68) in one call, medians and rule on
        the device; returns (steps taken, median kurtosis after every step)."""
        taken = C.c_int(0)
        med = np.empty(int(maxnsteps))
        check(self.lib.cna_nam_auto(self.h, int(maxnsteps), C.byref(taken), ptr(med)), 'cna_nam_auto')
        return taken.value, med[:taken.value]

    def nam_auto_launch(self, maxnsteps=15):
        """First half of nam_auto(): queue the walk and return at once.  The verdict is collected by
        nam_auto_finish() or by whatever engine call next reads the NAM."""
        check(self.lib.cna_nam_auto_launch(self.h, int(maxnsteps)), 'cna_nam_auto_launch')
        self._auto_max = int(maxnsteps)

    def nam_auto_finish(self):
        taken = C.c_int(0)
        med = np.empty(self._auto_max)
        check(self.lib.cna_nam_auto_finish(self.h, C.byref(taken), ptr(med)), 'cna_nam_auto_finish')
        return taken.value, med[:taken.value]

    def stat_median(self):
        """np.median of the per-cell statistic of the last kernel that made one, over all cells (or all
        kept cells, all ranks): exact radix select on the device, no cells-sized transfer."""
        m = C.c_double(0.0)
        check(self.lib.cna_stat_median(self.h, C.byref(m)), 'cna_stat_median')
        return m.value

    def stat_qc(self):
        """(median, threshold = max(6, 2 median), cells failing `kurtosis < threshold`) of the NAM's batch kurtosis
        (_nam.py:94-96), decided on the device; a count of zero means every cell is kept."""
        m, t, nd = C.c_double(0.0), C.c_double(0.0), C.c_int64(0)
        check(self.lib.cna_stat_qc(self.h, C.byref(m), C.byref(t), C.byref(nd)), 'cna_stat_qc')
        return m.value, t.value, nd.value

    def cell_stat(self, n_expected, nam_space=True):
        """Per-cell statistic of the last kernel that made one: over all cells in the caller's
        order (nam_space) or over the rows of X in device order (see x_stat())."""
        out = np.empty(int(n_expected))
        check(self.lib.cna_fetch_cell_stat(self.h, ptr(out), int(n_expected)), 'cna_fetch_cell_stat')
        return self.cells_to_user(out) if nam_space else out

    def load_cell_stat(self, v):
        """For tests: v (one float64 per cell of the resident graph) becomes the NAM-space per-cell statistic, as it
        stands -- stat_median() / stat_qc() then work on values of the caller's choosing.  cell_stat() hands the vector
        back through the device cell order: compare sorted, or undo that with cells_to_device()."""
        v = _f64(v)
        if v.ndim != 1:
            raise ValueError('the per-cell statistic is a vector')
        check(self.lib.cna_load_cell_stat(self.h, ptr(v), len(v)), 'cna_load_cell_stat')

    # ---------------------------------------------------------------- dense diffusion
    def dense_load(self, s_local):
        s_local = _f64(s_local)
        if s_local.ndim != 2 or s_local.shape[0] != self.n_local:
            raise ValueError('dense state must be (local cells) x m')
        check(self.lib.cna_dense_load(self.h, ptr(s_local), s_local.shape[1]), 'cna_dense_load')
        self._dense_m = s_local.shape[1]

    def dense_step(self):
        check(self.lib.cna_dense_step(self.h), 'cna_dense_step')

    def dense_fetch(self):
        out = np.empty((self.n_local, self._dense_m))
        check(self.lib.cna_dense_fetch(self.h, ptr(out)), 'cna_dense_fetch')
        return out

    # ---------------------------------------------------------------- QC / selection
    def batch_kurtosis(self, which, batch_codes, n_batches):
        bc = np.ascontiguousarray(batch_codes, dtype=np.int32)
        check(self.lib.cna_batch_kurtosis(self.h, which, ptr(bc), int(n_batches)), 'cna_batch_kurtosis')

    def zero_variance(self, colmap):
        cm = None if colmap is None else np.ascontiguousarray(colmap, dtype=np.int32)
        flags = np.zeros(self.n, dtype=np.uint8)
        nz = C.c_int64(0)
        check(self.lib.cna_zero_variance(self.h, ptr(cm), 0 if cm is None else len(cm), ptr(flags), C.byref(nz)),
              'cna_zero_variance')
        return self.cells_to_user(flags.astype(bool)), nz.value

    def _selection(self, keep_global):
        self._x_is_selection = True
        if keep_global is None:
            self._keep_dev = None
            self._kept_order_cache = None
            self.x_rows_total = self.n
            return None, 0
        idx = self.local_keep(keep_global)
        self.x_rows_total = int(np.count_nonzero(self._keep_dev))
        return idx, len(idx)

    def select(self, keep_global, colmap):
        """keep_global: bool mask over all cells (or None = all); colmap: NAM column per output column."""
        cm = None if colmap is None else np.ascontiguousarray(colmap, dtype=np.int32)
        idx, nk = self._selection(keep_global)
        check(self.lib.cna_select(self.h, ptr(idx), nk, ptr(cm), 0 if cm is None else len(cm)), 'cna_select')
        self.x_epoch += 1

    def set_resid_factors(self, Cmat, W):
        """The next select_standardized() also residualises: M = I - Cmat.W applied between centring and
        the division by the std (one pass over the NAM for selection + residualisation + standardisation)."""
        Cmat, W = _f64(Cmat), _f64(W)
        check(self.lib.cna_set_resid_factors(self.h, ptr(Cmat), ptr(W), int(Cmat.shape[1]), int(Cmat.shape[0])),
              'cna_set_resid_factors')

    def clear_resid_factors(self):
        check(self.lib.cna_set_resid_factors(self.h, None, None, 0, max(int(self.N), 1)), 'cna_set_resid_factors')

    def select_checked(self, keep_global, colmap):
        """select() and, in the same pass, the number of selected cells with zero variance over the
        selected samples (non-zero: redo with zero_variance() + select())."""
        cm = None if colmap is None else np.ascontiguousarray(colmap, dtype=np.int32)
        idx, nk = self._selection(keep_global)
        nz = C.c_int64(0)
        check(self.lib.cna_select_checked(self.h, ptr(idx), nk, ptr(cm), 0 if cm is None else len(cm), C.byref(nz)),
              'cna_select_checked')
        self.x_epoch += 1
        return nz.value

    def select_standardized(self, keep_global, colmap, y=None, fuse_null=0, null_ready=None):
        """select() + centre + divide by std in one pass (M = I); returns the number of selected
        cells with zero variance (non-zero: redo with zero_variance()/select()).  With ``y`` (the
        standardised phenotype in the selected samples' order) the neighbourhood coefficients are
        taken in the same pass and (n_zero, max |ncorrs|) is returned -- ncorrs(y) is then done.
        ``fuse_null`` = P > 0 (with y): when no cell has zero variance the same call also queues what
        would follow from values it returns -- gram_launch(), the thresholds of the local null from
        max|ncorrs|, null_local_prepare(P, ...) and percell_coef_launch(); those methods then find
        their work done (they compare arguments) and return at once.  ``null_ready``: a callable asked right before
        the call whether the conditioned phenotypes of this analysis are on the device already (condition() has
        returned); the prepared local-null pass is then launched in the same call (columns 1 .. P)."""
        cm = None if colmap is None else np.ascontiguousarray(colmap, dtype=np.int32)
        idx, nk = self._selection(keep_global)
        nz = C.c_int64(0)
        m = C.c_double(0.0)
        yv = None if y is None else _f64(y)
        self.null_local_discard()       # (a pass left behind by an analysis that raised after its launch)
        if yv is not None and fuse_null > 0:
            T, gq, cq, nl = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
            thr = np.empty(512)
            # null_ready: a callable (the caller's own word, now) or an int32 array of one element that the library's
            # draw thread sets once its conditioning has returned (read by the C call at the moment it matters)
            flag = null_ready if isinstance(null_ready, np.ndarray) else None
            col0 = 1 if (flag is not None or (null_ready is not None and null_ready())) else -1
            check(self.lib.cna_select_standardized_fused(self.h, ptr(idx), nk, ptr(cm), 0 if cm is None else len(cm),
                                                         C.byref(nz), ptr(yv), C.byref(m), int(fuse_null), C.byref(T),
                                                         ptr(thr), C.byref(gq), C.byref(cq), col0, ptr(flag), C.byref(nl)),
                  'cna_select_standardized_fused')
            self.x_epoch += 1
            self._fused = dict(epoch=self.x_epoch, P=int(fuse_null), thr=thr[:T.value], gram=bool(gq.value),
                               coef=bool(cq.value), prepared=T.value > 0 and not nl.value, null=bool(nl.value))
            if gq.value:
                self._gram_cols = self.N if cm is None else len(cm)
            if T.value:
                self._null_T, self._null_obs = T.value, True
            return nz.value, m.value
        check(self.lib.cna_select_standardized(self.h, ptr(idx), nk, ptr(cm), 0 if cm is None else len(cm),
                                               C.byref(nz), ptr(yv), C.byref(m)), 'cna_select_standardized')
        self.x_epoch += 1
        return nz.value if y is None else (nz.value, m.value)

    def _fused_done(self, what):
        """True once: the fused selection call already issued `what` for the current working matrix."""
        f = getattr(self, '_fused', None)
        if f is None or f['epoch'] != self.x_epoch or not f.get(what):
            return False
        f[what] = False
        return True

    def upload_x(self, x_local):
        x_local = _f64(x_local)
        check(self.lib.cna_upload_x(self.h, ptr(x_local), x_local.shape[0], x_local.shape[1]), 'cna_upload_x')
        self.x_rows_total = x_local.shape[0]   # single-rank use (cna.tl.svd_nam)
        self._x_is_selection = False
        self.x_epoch += 1

    # ---------------------------------------------------------------- residualise + PCA
    def resid_apply(self, M, center):
        M = None if M is None else _f64(M)
        check(self.lib.cna_resid_apply(self.h, ptr(M), int(bool(center))), 'cna_resid_apply')

    def resid_lowrank(self, Cmat, W, center=True, standardize=False, y=None):
        """X <- (X - mean).M^T [/ std] for M = I - Cmat.W (Cmat: N x r, W: r x N) in one row-local pass; with
        `y` also the neighbourhood coefficients, returning max |ncorrs| (else None)."""
        Cmat, W = _f64(Cmat), _f64(W)
        r = Cmat.shape[1]
        if W.shape != (r, Cmat.shape[0]):
            raise ValueError('W must be r x N for an N x r C')
        yv = None if y is None else _f64(y)
        m = C.c_double(0.0)
        check(self.lib.cna_resid_lowrank(self.h, ptr(Cmat), ptr(W), int(r), int(bool(center)), int(bool(standardize)),
                                         ptr(yv), C.byref(m)), 'cna_resid_lowrank')
        return m.value if y is not None else None

    def resid_lowrank_bk(self, Cmat, W, y, batch_codes, n_batches):
        """One ridge in one pass: X <- (X - mean).M^T for M = I - Cmat.W, its batch kurtosis and the median of that
        (on the device), then / std and the coefficients X.y/N.  Returns (max |ncorrs|, median batch kurtosis); when
        the median is > 6 the caller must restore X before going on with the next ridge."""
        Cmat, W, yv = _f64(Cmat), _f64(W), _f64(y)
        r = Cmat.shape[1]
        bc = np.ascontiguousarray(batch_codes, dtype=np.int32)
        m, med = C.c_double(0.0), C.c_double(0.0)
        check(self.lib.cna_resid_lowrank_bk(self.h, ptr(Cmat), ptr(W), int(r), ptr(yv), C.byref(m), ptr(bc), int(n_batches),
                                            C.byref(med)), 'cna_resid_lowrank_bk')
        return m.value, med.value

    def select_resid_bk(self, Cmat, W, y, batch_codes, n_batches):
        """Selection (every cell, samples in place) + QC + the first ridge in ONE pass over the NAM (cna_select_resid_bk).
        -> None (shape not covered, nothing queued) or (rows failing the QC, rows of zero variance, max |ncorrs|, median
        batch kurtosis of the residualised rows); X is final when the first two are 0 and the median is <= 6."""
        Cmat, W, yv = _f64(Cmat), _f64(W), _f64(y)
        bc = np.ascontiguousarray(batch_codes, dtype=np.int32)
        if Cmat.ndim != 2 or W.shape != (Cmat.shape[1], Cmat.shape[0]) or len(yv) != Cmat.shape[0] or len(bc) != len(yv):
            return None
        m, med = C.c_double(0.0), C.c_double(0.0)
        nq, nz, done = C.c_int64(0), C.c_int64(0), C.c_int(0)
        self.null_local_discard()
        check(self.lib.cna_select_resid_bk(self.h, ptr(Cmat), ptr(W), int(Cmat.shape[1]), ptr(yv), C.byref(m), ptr(bc), int(n_batches),
                                           C.byref(med), C.byref(nq), C.byref(nz), C.byref(done)), 'cna_select_resid_bk')
        if not done.value:
            return None
        self._selection(None)
        self.x_epoch += 1
        return nq.value, nz.value, m.value, med.value

    def standardize(self, center=False):
        check(self.lib.cna_standardize(self.h, int(bool(center))), 'cna_standardize')

    def gram(self):
        rows, cols = self.matrix_shape(MAT_X)
        G = np.empty((cols, cols))
        check(self.lib.cna_gram(self.h, ptr(G)), 'cna_gram')
        return G

    def gram_launch(self):
        if self._fused_done('gram'):
            return
        check(self.lib.cna_gram_launch(self.h), 'cna_gram_launch')
        self._gram_cols = self.matrix_shape(MAT_X)[1]

    def gram_fetch(self):
        G = np.empty((self._gram_cols, self._gram_cols))
        check(self.lib.cna_gram_fetch(self.h, ptr(G)), 'cna_gram_fetch')
        return G

    def gram_held(self):
        """The Gram matrix X^T X of the current working matrix as the library still holds it from the last launch (an
        analysis leaves it there), else launched now -- on the device either way, never from a fetched X."""
        cols = self.matrix_shape(MAT_X)[1]
        G = np.empty((cols, cols))
        if self.lib.cna_gram_fetch(self.h, ptr(G)) != 0:       # voided, or of another order: take it again
            check(self.lib.cna_gram(self.h, ptr(G)), 'cna_gram')
        self._gram_cols = cols
        return G

    def gram_pcs_tests(self, ks, r, native=True, resid_tol=1e-12, gap_tol=1e-6):
        """gram_fetch(), the leading max(ks) eigenpairs on the host and -- when the library's own solver is accepted
        (tools/_nam.py:_top_pcs_native's rule) -- global_test_launch(), in ONE call without the interpreter in between.
        Returns (G, U or None, queued): queued -> collect with global_test_fetch(); else the caller finds the
        eigenvectors elsewhere and launches the tests itself."""
        ks = np.ascontiguousarray(ks, dtype=np.int32)
        kmax = int(ks.max())
        n = self._gram_cols
        G = np.empty((n, n))
        U = np.empty((n, max(kmax, 1)))
        ok = C.c_int(0)
        check(self.lib.cna_gram_pcs_tests(self.h, kmax, ptr(ks), len(ks), int(r), int(bool(native)), float(resid_tol), float(gap_tol),
                                          ptr(G), ptr(U), C.byref(ok)), 'cna_gram_pcs_tests')
        return G, (U if ok.value else None), bool(ok.value)

    def project(self, W):
        W = _f64(W)
        rows, cols = self.matrix_shape(MAT_X)
        out = np.empty((rows, W.shape[1]))
        check(self.lib.cna_project(self.h, ptr(W), W.shape[1], ptr(out)), 'cna_project')
        return out

    # ---------------------------------------------------------------- association
    def x_identity_resident(self):
        """True when X on the device is the standardised NAM of the resident walk for "every cell, samples in place,
        nothing regressed out": a further analysis of the dataset with that selection keeps it (ncorrs(y) next)."""
        yes = C.c_int(0)
        check(self.lib.cna_x_identity(self.h, C.byref(yes)), 'cna_x_identity')
        return bool(yes.value)

    def ncorrs(self, y, fetch=False):
        y = _f64(y)
        rows, cols = self.matrix_shape(MAT_X)
        out = np.empty(rows) if fetch else None
        m = C.c_double(0.0)
        check(self.lib.cna_ncorrs(self.h, ptr(y), ptr(out), C.byref(m)), 'cna_ncorrs')
        if fetch and (self.nranks == 1 or self.view_local):
            out = self.kept_to_user(out)     # kept cells (of the caller's view) in the caller's order
        return out, m.value

    def null_local(self, Yc, edges):
        Yc = _f64(Yc)
        edges = _f64(edges)
        P, T = Yc.shape[1], len(edges)
        tails = np.empty((P, T), dtype=np.int64)
        check(self.lib.cna_null_local(self.h, ptr(Yc), P, ptr(edges), T, ptr(tails)), 'cna_null_local')
        return tails

    def condition(self, M, Y):
        """Zc = M.Y / std(M.Y, ddof=1) per column, kept on the device (column 0: observed phenotype).
        Sample space only and on the second stream: may be issued while the diffusion is running."""
        M, Y = _f64(M), _f64(Y)
        if M.shape != (Y.shape[0], Y.shape[0]):
            raise ValueError('M must be square with one row per phenotype entry')
        check(self.lib.cna_condition_phenotypes(self.h, ptr(M), ptr(Y), Y.shape[0], Y.shape[1]),
              'cna_condition_phenotypes')
        self._zc_cols = Y.shape[1]

    def null_local_resident(self, col0, P, edges, sums_only=False):
        """Tail counts of the local null on resident columns: P x T matrix, or (sums_only) its sum
        over permutations, which is all the FDR formula needs."""
        edges = _f64(edges)
        T = len(edges)
        tails = None if sums_only else np.empty((int(P), T), dtype=np.int64)
        sums = np.empty(T, dtype=np.int64) if sums_only else None
        check(self.lib.cna_null_local_resident(self.h, int(col0), int(P), ptr(edges), T, ptr(tails), ptr(sums)),
              'cna_null_local_resident')
        return sums if sums_only else tails

    def null_local_i8_stats(self):
        """(integer path used, outputs rechecked in f64, fell back to the f64 kernel) of the last sums-only pass."""
        used, fb = C.c_int(0), C.c_int(0)
        rc = C.c_int64(0)
        check(self.lib.cna_null_local_i8_stats(self.h, C.byref(used), C.byref(rc), C.byref(fb)), 'cna_null_local_i8_stats')
        return bool(used.value), int(rc.value), bool(fb.value)

    def null_local_prepare(self, P, edges, thr=None):
        """First half of null_local_launch: needs the thresholds only (exact cuts, observed counts);
        finish with null_local_launch(col0, P, None)."""
        edges = _f64(edges)
        thr = None if thr is None else _f64(thr)
        f = getattr(self, '_fused', None)
        if (thr is not None and f is not None and f['epoch'] == self.x_epoch and f['prepared'] and f['P'] == int(P)
                and np.array_equal(f['thr'], thr)):
            f['prepared'] = False             # the fused selection call prepared exactly this pass
            return
        if f is not None and f['epoch'] == self.x_epoch and f.get('null'):
            if thr is not None and f['P'] == int(P) and np.array_equal(f['thr'], thr):
                return                        # ... and launched it as well (null_local_launch finds that out)
            # the fused call's own thresholds are not the caller's (never seen; numpy's arange and its C restatement
            # are compared in the tests): collect that pass and start over
            f['null'] = False
            self._null_T, self._null_obs = len(f['thr']), True
            self.null_local_fetch()
        if f is not None:
            f['coef'] = False                 # a fresh prepare: whatever rode along with the fused one is void
        check(self.lib.cna_null_local_prepare(self.h, int(P), ptr(edges), len(edges), 0, ptr(thr)),
              'cna_null_local_prepare')
        self._null_T = len(edges)
        self._null_obs = thr is not None

    def null_local_launch(self, col0, P, edges, thr=None):
        """Queue a local-null pass on resident columns; collect with null_local_fetch().  With `thr`
        the threshold counts of the observed coefficients (obs_counts) are queued in front of it."""
        if edges is None:                       # prepared pass
            if int(col0) == 1 and self._fused_done('null'):
                return                          # the fused selection call launched it already
            check(self.lib.cna_null_local_launch(self.h, int(col0), int(P), None, self._null_T, 0, None),
                  'cna_null_local_launch')
            return
        edges = _f64(edges)
        thr = None if thr is None else _f64(thr)
        check(self.lib.cna_null_local_launch(self.h, int(col0), int(P), ptr(edges), len(edges), 0, ptr(thr)),
              'cna_null_local_launch')
        self._null_T = len(edges)
        self._null_obs = thr is not None

    def null_local_fetch(self):
        """Tail sums of the pending pass, or (tail sums, ranks, num_detected) when it was launched with thr."""
        T = self._null_T
        sums = np.empty(T, dtype=np.int64)
        if not self._null_obs:
            check(self.lib.cna_null_local_fetch(self.h, None, ptr(sums), None, None), 'cna_null_local_fetch')
            return sums
        ranks, numdet = np.empty(T, dtype=np.int64), np.empty(T, dtype=np.int64)
        check(self.lib.cna_null_local_fetch(self.h, None, ptr(sums), ptr(ranks), ptr(numdet)), 'cna_null_local_fetch')
        return sums, ranks, numdet

    def null_local_discard(self):
        """Drop a local-null pass that was launched (here or by the fused selection call) and never fetched -- the
        caller raised in between -- and whatever else the fused call queued for an analysis that will not happen.
        No-op when nothing is pending; called on the error paths of association() and before every new selection."""
        self._fused = None
        check(self.lib.cna_null_local_discard(self.h), 'cna_null_local_discard')

    def global_test(self, U, ks, r):
        """min-p F-test of every resident phenotype column -> (index into ks, p, r2) arrays."""
        ks = np.ascontiguousarray(ks, dtype=np.int32)
        kmax = int(ks.max())
        Uk = _f64(U[:, :kmax])
        P = self._zc_cols
        minp, r2, kidx = np.empty(P), np.empty(P), np.empty(P, dtype=np.int32)
        check(self.lib.cna_global_test(self.h, ptr(Uk), kmax, ptr(ks), len(ks), int(r), ptr(minp), ptr(r2), ptr(kidx)),
              'cna_global_test')
        return kidx, minp, r2

    def global_test_launch(self, U, ks, r):
        """First half of global_test(): queue it and return; collect with global_test_fetch()."""
        ks = np.ascontiguousarray(ks, dtype=np.int32)
        kmax = int(ks.max())
        Uk = _f64(U[:, :kmax])
        check(self.lib.cna_global_test_launch(self.h, ptr(Uk), kmax, ptr(ks), len(ks), int(r)), 'cna_global_test_launch')

    def global_test_fetch(self):
        P = self._zc_cols
        minp, r2, kidx = np.empty(P), np.empty(P), np.empty(P, dtype=np.int32)
        check(self.lib.cna_global_test_fetch(self.h, ptr(minp), ptr(r2), ptr(kidx)), 'cna_global_test_fetch')
        return kidx, minp, r2

    def global_test_discard(self):
        """Collect and drop a queued global test nobody will fetch (error paths); no-op when none is pending."""
        try:
            self.global_test_fetch()
        except _ffi.CnaHipError:
            pass

    # ---------------------------------------------------------------- the fixed-shape analysis in two calls
    def assoc_begin(self, nsteps, y_hint=None):
        """Queue the walk of a fixed-shape analysis (cna_assoc_begin): `nsteps` steps (0: the NAM on the device is
        kept), with `y_hint` the last step also does the selection pass (nam_select_hint).  Returns at once."""
        yv = None if y_hint is None else _f64(y_hint)
        check(self.lib.cna_assoc_begin(self.h, int(nsteps), ptr(yv), 0 if yv is None else len(yv)), 'cna_assoc_begin')
        if yv is not None and nsteps >= 2:
            self.x_epoch += 1             # (that step overwrites the working matrix: see nam_select_hint)

    def assoc_begin_part(self, first, count, total, y_hint=None):
        """Steps first .. first + count - 1 (0-based) of a walk of `total` steps (cna_assoc_begin_part); y_hint goes with
        the part that holds the last step."""
        yv = None if y_hint is None else _f64(y_hint)
        check(self.lib.cna_assoc_begin_part(self.h, int(first), int(count), int(total), ptr(yv), 0 if yv is None else len(yv)),
              'cna_assoc_begin_part')
        if yv is not None and total >= 2 and first + count == total:
            self.x_epoch += 1

    def assoc_finish(self, y, M, ks, Nnull, table, colmap=None, Cmat=None, W=None, draw_pending=False, conditioned=False,
                     coef_dst=None, fdr_dst=None, coef_first=False, copy_threads=1, native_eig=True, resid_tol=1e-12,
                     gap_tol=1e-6, run_steps=None, y_hint=None, verify=(), verify_threads=1):
        """Selection (+ projector) -> Gram -> eigenpairs -> F-tests, conditioned phenotypes -> local null -> FDR table ->
        per-cell columns, in ONE blocking library call (cna_assoc_finish; include/cna_hip.h).  Returns a dict: status,
        n_zero, maxabs, thr, tail_sums, ranks, num_detected, fdr, runmin, G, U (None unless accepted), minp / r2 / kidx
        (None when status is ASSOC_NEED_PCS), coef / fdr (views of pinned buffers, or the caller's own storage).
        run_steps = nsteps: the walk is queued by the same call (cna_assoc_run = assoc_begin(nsteps, y_hint) + this)."""
        a = _ffi.AssocArgs()
        keep = []                                     # arrays the struct points to

        def P(arr):
            keep.append(arr)
            return arr.ctypes.data
        yv, Mv = _f64(y), _f64(M)
        N = len(yv)
        ksv = np.ascontiguousarray(ks, dtype=np.int32)
        kmax = int(ksv.max())
        P1 = int(Nnull) + 1
        if Mv.shape != (N, N) or table.shape != (N, P1) or table.dtype != np.float64 or not table.flags.c_contiguous:
            raise ValueError('assoc_finish: M must be N x N and table a C-contiguous float64 N x (Nnull + 1) matrix')
        a.colmap = None if colmap is None else P(np.ascontiguousarray(colmap, dtype=np.int32))
        a.n_sel, a.y, a.M = N, P(yv), P(Mv)
        if Cmat is not None and W is not None and np.shape(Cmat)[1] > 0:
            Cv, Wv = _f64(Cmat), _f64(W)
            if Cv.shape[0] != N or Wv.shape != (Cv.shape[1], N):
                raise ValueError('assoc_finish: C must be N x r and W r x N')
            a.r, a.resid_C, a.resid_W = Cv.shape[1], P(Cv), P(Wv)
        a.ks, a.K, a.Nnull = P(ksv), len(ksv), int(Nnull)
        a.table = P(table)
        a.draw_pending, a.conditioned = int(bool(draw_pending)), int(bool(conditioned))
        a.use_native_eig, a.coef_first = int(bool(native_eig)), int(bool(coef_first))
        a.resid_tol, a.gap_tol = float(resid_tol), float(gap_tol)
        if coef_dst is not None and fdr_dst is not None:
            a.coef_dst, a.fdr_dst, a.n_dst = coef_dst.ctypes.data, fdr_dst.ctypes.data, len(coef_dst)
            keep += [coef_dst, fdr_dst]
        a.copy_threads = int(copy_threads)
        # verify: [(array, 64-bit content hash it must still have)], checked by the library while the device works
        a.n_verify = len(verify)
        for i, (arr, hv) in enumerate(verify):
            a.verify_ptr[i], a.verify_bytes[i], a.verify_hash[i] = arr.ctypes.data, arr.nbytes, int(hv)
            keep.append(arr)
        a.verify_threads = int(verify_threads)
        G, U = np.empty((N, N)), np.empty((N, max(kmax, 1)))
        minp, r2, kidx = np.empty(P1), np.empty(P1), np.empty(P1, dtype=np.int32)
        a.G, a.U, a.minp, a.r2, a.kidx = P(G), P(U), P(minp), P(r2), P(kidx)
        if self._assoc_out is None:
            o = _ffi.AssocOut()
            raw = np.frombuffer(o, dtype=np.uint8)    # numpy views of the struct's arrays (a ctypes slice makes a list)
            views = {f: raw[getattr(_ffi.AssocOut, f).offset:][:8 * _ffi.ASSOC_MAXT].view(np.float64 if f in ('thr', 'fdr', 'runmin') else np.int64)
                     for f in ('thr', 'fdr', 'runmin', 'tail_sums', 'ranks', 'num_detected')}
            self._assoc_out = (o, views)
        o, ov = self._assoc_out
        # bookkeeping of what the call replaces on the device, before it can fail half-way
        self._fused = None
        self._selection(None)
        self.x_epoch += 1
        self._gram_cols = N
        self._zc_cols = P1
        if run_steps is None:
            check(self.lib.cna_assoc_finish(self.h, C.byref(a), C.byref(o)), 'cna_assoc_finish')
        else:
            hv = None if y_hint is None else _f64(y_hint)
            check(self.lib.cna_assoc_run(self.h, int(run_steps), ptr(hv), 0 if hv is None else len(hv), C.byref(a), C.byref(o)),
                  'cna_assoc_run')
        T = int(o.T)
        self._null_T, self._null_obs = T, True
        status = o.status
        out = dict(status=status, n_zero=o.n_zero, maxabs=o.max_abs, T=T, G=G, null_fused=o.null_fused,
                   U=U if o.eig_accepted else None, coef_in_dst=o.coef_in_dst, fdr_in_dst=o.fdr_in_dst, t_ms=o.t_ms)
        if status in (_ffi.ASSOC_GENERAL, _ffi.ASSOC_STALE):
            return out
        # (views of the call's own output block, valid until the next assoc_finish: a caller that keeps them copies them)
        for f, v in ov.items():
            out[f] = v[:T]
        if status == _ffi.ASSOC_DONE:
            out['minp'], out['r2'], out['kidx'] = minp, r2, kidx
        out['coef'] = coef_dst if o.coef_in_dst else (self._pinned_view(C.c_void_p(o.coef_ptr)) if o.coef_ptr else None)
        out['fdr_col'] = fdr_dst if o.fdr_in_dst else (self._pinned_view(C.c_void_p(o.fdr_ptr)) if o.fdr_ptr else None)
        return out

    @property
    def last_assoc_t_ms(self):
        """Stage times of the last cna_assoc_finish (ms from its entry; include/cna_hip.h: cna_assoc_out.t_ms), or None."""
        return None if self._assoc_out is None else list(self._assoc_out[0].t_ms)

    def obs_counts(self, edges, thr):
        edges, thr = _f64(edges), _f64(thr)
        T = len(thr)
        ranks = np.empty(T, dtype=np.int64)
        numdet = np.empty(T, dtype=np.int64)
        check(self.lib.cna_obs_counts(self.h, ptr(edges), ptr(thr), T, ptr(ranks), ptr(numdet)), 'cna_obs_counts')
        return ranks, numdet

    def percell(self, thr=None, runmin=None):
        """Per-cell coefficient (NaN for dropped cells) and FDR columns over all cells, caller's order.
        The arrays are views of pinned buffers owned by the engine: valid until the next percell()
        -- copy them (assigning to a DataFrame column does) before running another analysis."""
        cp, fp = C.c_void_p(), C.c_void_p()
        if thr is None:
            check(self.lib.cna_percell_fdr_pinned(self.h, None, None, 0, C.byref(cp), None), 'cna_percell_fdr_pinned')
            return self._pinned_view(cp), None
        thr, runmin = _f64(thr), _f64(runmin)
        check(self.lib.cna_percell_fdr_pinned(self.h, ptr(thr), ptr(runmin), len(thr), C.byref(cp), C.byref(fp)),
              'cna_percell_fdr_pinned')
        return self._pinned_view(cp), self._pinned_view(fp)

    def percell_coef_launch(self):
        """Queue the per-cell coefficient column ahead of the local-null kernel (it only needs the
        observed phenotype); False when this engine assembles per-cell outputs across ranks."""
        if (self.nranks > 1 or self._has_comm) and not self.view_local:
            return False
        if self._fused_done('coef'):
            return True
        check(self.lib.cna_percell_coef_launch(self.h), 'cna_percell_coef_launch')
        return True

    def percell_coef_wait(self):
        """The coefficient column queued by percell_coef_launch (pinned view, see percell()); callable
        from a helper thread."""
        cp = C.c_void_p()
        check(self.lib.cna_percell_coef_wait(self.h, C.byref(cp)), 'cna_percell_coef_wait')
        return self._pinned_view(cp)

    def percell_fdr_copy_early(self, dst, threads=4):
        """Copy the FDR column of the pending local-null pass into `dst` (contiguous float64, all cells) once the
        device has delivered it; for a helper thread.  False: not applicable, nothing copied."""
        done = C.c_int(0)
        check(self.lib.cna_percell_fdr_copy_early(self.h, dst.ctypes.data, dst.shape[0], int(threads), C.byref(done)),
              'cna_percell_fdr_copy_early')
        return bool(done.value)

    def percell_fdr_copied_early(self):
        """True when the FDR column percell() last returned is the one percell_fdr_copy_early() copied."""
        yes = C.c_int(0)
        check(self.lib.cna_percell_fdr_copied_early(self.h, C.byref(yes)), 'cna_percell_fdr_copied_early')
        return bool(yes.value)

    def _pinned_view(self, p):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_double)), shape=(self.n,))

    # ---------------------------------------------------------------- D2H
    def matrix_shape(self, which):
        r, c = C.c_int64(0), C.c_int(0)
        check(self.lib.cna_matrix_shape(self.h, which, C.byref(r), C.byref(c)), 'cna_matrix_shape')
        return r.value, c.value

    def fetch_matrix(self, which, transposed=False):
        rows, cols = self.matrix_shape(which)
        out = np.empty((cols, rows) if transposed else (rows, cols))
        check(self.lib.cna_fetch_matrix(self.h, which, ptr(out), int(bool(transposed))), 'cna_fetch_matrix')
        return out

    def nam_padding(self):
        """For tests: the padding columns N <= col < ld of the NAM's rows as they stand on the device (local rows x
        (ld - N), device cell order); every walk step writes zeros there.  The NAM only, not the walk's state buffers."""
        pad = C.c_int(0)
        check(self.lib.cna_fetch_nam_padding(self.h, None, C.byref(pad)), 'cna_fetch_nam_padding')
        out = np.empty((self.n_local, pad.value))
        if out.size:
            check(self.lib.cna_fetch_nam_padding(self.h, ptr(out), C.byref(pad)), 'cna_fetch_nam_padding')
        return out

    def fetch_rows(self, which, rows=None, cols=None, transposed=False):
        """out[i, j] = M[rows[i], cols[j]] (None = all, in order) picked and ordered on the device;
        transposed=True returns the (columns x rows) layout.  which: MAT_NAM, MAT_X or MAT_PROJ."""
        if which == _ffi.MAT_PROJ:
            have, width = self._proj_shape
        else:
            have, width = self.matrix_shape(which)
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        cm = None if cols is None else np.ascontiguousarray(cols, dtype=np.int32)
        n_out = have if r is None else len(r)
        n_cols = width if cm is None else len(cm)
        out = np.empty((n_cols, n_out) if transposed else (n_out, n_cols))
        check(self.lib.cna_fetch_rows(self.h, which, ptr(r), n_out, ptr(cm), n_cols, ptr(out), int(bool(transposed))),
              'cna_fetch_rows')
        return out

    def project_keep(self, W):
        """X.W left on the device; read it with fetch_rows(MAT_PROJ, ...)."""
        W = _f64(W)
        check(self.lib.cna_project_keep(self.h, ptr(W), W.shape[1]), 'cna_project_keep')
        self._proj_shape = (self.matrix_shape(MAT_X)[0], W.shape[1])

    def x_rows_global(self):
        """Rows of the working matrix over all ranks (a collective in the local view)."""
        if not self.view_local or self.nranks == 1:
            return self.x_rows_total
        return int(self.allgather_fixed([self.x_rows_total]).sum())

    def allgather_fixed(self, values):
        """(nranks x len(values)) int64: the same-length vector of every rank, one collective."""
        a = np.ascontiguousarray(values, dtype=np.int64)
        if self.nranks == 1:
            return a.reshape(1, -1).copy()
        out = np.empty(self.nranks * len(a), dtype=np.int64)
        check(self.lib.cna_allgather_host(self.h, ptr(a), len(a), ptr(out), len(out)), 'cna_allgather_host')
        return out.reshape(self.nranks, len(a))

    def allgather_objects(self, obj):
        """[obj of rank 0, obj of rank 1, ...] for small picklable host objects (sample labels)."""
        import pickle
        if self.nranks == 1:
            return [obj]
        blob = pickle.dumps(obj, protocol=4)
        pad = (-len(blob)) % 8
        words = np.frombuffer(blob + b'\0' * pad, dtype=np.int64)
        sizes = self.allgather_fixed([len(blob), len(words)])
        flat = self._allgather_i64(words)
        out, off = [], 0
        for nbytes, nwords in sizes:
            out.append(pickle.loads(flat[off:off + nwords].tobytes()[:nbytes]))
            off += nwords
        return out

    def gather_rows_host(self, local, n_total):
        """Row blocks of every rank, concatenated in rank order (no-op on one GPU)."""
        local = _f64(local)
        if self.nranks == 1:
            return local
        cols = local.shape[1] if local.ndim == 2 else 1
        out = np.empty((int(n_total), cols) if local.ndim == 2 else int(n_total))
        check(self.lib.cna_allgather_host(self.h, ptr(local), local.size, ptr(out), out.size), 'cna_allgather_host')
        return out

    def _allgather_i64(self, a):
        """Concatenation over ranks of int64 vectors of differing lengths (graph preparation)."""
        a = np.ascontiguousarray(a, dtype=np.int64)
        if self.nranks == 1:
            return a.copy()
        sizes = np.zeros(self.nranks)
        check(self.lib.cna_allgather_host(self.h, ptr(np.array([float(len(a))])), 1, ptr(sizes), self.nranks),
              'cna_allgather_host')
        out = np.empty(int(sizes.sum()), dtype=np.int64)
        check(self.lib.cna_allgather_host(self.h, ptr(a), len(a), ptr(out), len(out)), 'cna_allgather_host')
        return out

    # ---------------------------------------------------------------- expression matrix (tools._genes.gene_corr)
    @staticmethod
    def _expr_arrays(X):
        return (X,) if isinstance(X, np.ndarray) else (X.data, X.indices, X.indptr)

    def _expr_buffers(self, X):
        return tuple(a.ctypes.data for a in self._expr_arrays(X))

    def _expr_ident(self, X):
        if not isinstance(X, np.ndarray):
            return (X.format,) + self._ident(X)
        return ('dense', X.shape, str(X.dtype), id(X), X.ctypes.data)

    def _expr_quick_key(self, X):
        """Cheap identity of an expression matrix, like `_quick_key` of a graph (which serves the sparse formats as it
        is): object, buffers, sizes, dtypes and a hash of three 64 KB windows.  Necessary, not sufficient."""
        if not isinstance(X, np.ndarray):
            return (X.format,) + self._quick_key(X)
        flat = X.reshape(-1)
        w = 16384
        mid = max(0, flat.size // 2 - w // 2)
        parts = [slice(0, w), slice(mid, mid + w), slice(max(0, flat.size - w), flat.size)]
        return self._expr_ident(X) + tuple(self._hash(flat[p_], 1) for p_ in parts)

    def _expr_is_pinned(self, X):
        return (self._expr_pinned is not None and self._expr_pinned[0]() is X
                and self._expr_pinned[1] == self._expr_buffers(X))

    def pin_expression(self, X):
        """Promise that the expression matrix X will not be edited in place while it is resident: later calls then
        recognise it without hashing all of it (what a loop over many phenotypes of one dataset wants).
        `unpin_expression()` withdraws the promise."""
        if not isinstance(X, np.ndarray) and not sp.issparse(X):
            raise TypeError('pin_expression needs the matrix that is passed to gene_corr')
        self._expr_pinned = (weakref.ref(X), self._expr_buffers(X))

    def unpin_expression(self):
        self._expr_pinned = None

    def drop_expression(self):
        """Forget the resident expression matrix and free its device memory: the next call uploads afresh."""
        self._expr_key = self._expr_hash = self._expr_ref = None
        self._cross_memo = None
        self._cross_by_memo = None
        check(self.lib.cna_expr_drop(self.h), 'cna_expr_drop')

    def ensure_expression(self, X):
        """Upload the expression matrix (cells x genes, caller's cell order; already validated by tools._genes) unless
        this very matrix -- same object, same content -- is resident.  Content check as for the graph: the full hash of
        its arrays unless the matrix is pinned (`pin_expression`).  One matrix per engine: another one replaces it.
        Returns True when it went to the device."""
        same = self._expr_key is not None and self._expr_ref is not None and self._expr_ref() is X
        pinned = self._expr_is_pinned(X)
        if pinned and same:
            # pinned: the caller's promise replaces the content probes
            ident = self._expr_ident(X)
            if self._expr_key[:len(ident)] == ident:
                return False
        quick = self._expr_quick_key(X)
        full = None
        if same and self._expr_key == quick:
            if pinned:
                return False
            full = tuple(self._hash(a) for a in self._expr_arrays(X))
            if full == self._expr_hash:
                return False
        self._expr_key = self._expr_hash = self._expr_ref = None
        self._upload_expression(X)
        self._expr_key = quick
        self._expr_hash = full if full is not None else tuple(self._hash(a) for a in self._expr_arrays(X))
        try:
            self._expr_ref = weakref.ref(X)
        except TypeError:
            self._expr_ref = None
        return True

    def _upload_expression(self, X):
        n, g = X.shape
        if isinstance(X, np.ndarray):
            check(self.lib.cna_expr_upload_dense(self.h, ptr(X), n, g, int(X.dtype == np.float64)), 'cna_expr_upload_dense')
        else:
            M = X
            if not M.has_canonical_format:
                # duplicates add up and indices ascend, as toarray() would have it (a copy: the caller's matrix stays)
                M = M.copy()
                M.sum_duplicates()
            idt = np.int32 if M.indices.dtype == np.int32 and M.indptr.dtype == np.int32 else np.int64
            indptr = np.ascontiguousarray(M.indptr, dtype=idt)
            indices = np.ascontiguousarray(M.indices, dtype=idt)
            data = np.ascontiguousarray(M.data)
            check(self.lib.cna_expr_upload_sparse(self.h, ptr(indptr), ptr(indices), ptr(data), n, g, int(M.nnz),
                                                  indptr.dtype.itemsize, int(data.dtype == np.float64),
                                                  int(M.format == 'csc')), 'cna_expr_upload_sparse')

    def expression_shape(self):
        """What is resident: dict(n_cells, n_genes, nnz, format 'none' | 'dense' | 'gene-major', f64, uploads)."""
        n, g, nnz, up = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0)
        fmt, f64 = C.c_int(0), C.c_int(0)
        check(self.lib.cna_expr_shape(self.h, C.byref(n), C.byref(g), C.byref(nnz), C.byref(fmt), C.byref(f64), C.byref(up)),
              'cna_expr_shape')
        return dict(n_cells=n.value, n_genes=g.value, nnz=nnz.value, format=('none', 'dense', 'gene-major')[fmt.value],
                    f64=bool(f64.value), uploads=up.value)

    def gene_corr(self, V):
        """Pearson correlation of every gene of the resident expression matrix with every row of V (q x cells float64,
        caller's cell order, NaN = cell left out): q x genes float64 (cna_gene_corr)."""
        V = _f64(V)
        out = np.empty((V.shape[0], self.expression_shape()['n_genes']))
        check(self.lib.cna_gene_corr(self.h, ptr(V), V.shape[0], ptr(out)), 'cna_gene_corr')
        return out

    def nbhd_expr(self, genes, nsteps):
        """Numerators (cells x len(genes)) and denominator (cells) of the neighbourhood-mean expression of the chosen
        genes of the resident matrix after `nsteps` walk steps on the resident graph, float64, caller's cell order
        (cna_nbhd_expr).  Needs `ensure_graph`, `colsums` and `ensure_expression`; the walk's state and the NAM stay."""
        genes = np.ascontiguousarray(genes, dtype=np.int32)
        n = self.expression_shape()['n_cells']
        num = np.empty((n, genes.size))
        den = np.empty(n)
        check(self.lib.cna_nbhd_expr(self.h, ptr(genes), genes.size, int(nsteps), ptr(num), ptr(den)), 'cna_nbhd_expr')
        return num, den

    def gene_nbhd_corr(self, V, nsteps, timed=False):
        """Pearson correlation of the neighbourhood-mean expression of every gene with every row of V (q x cells float64,
        caller's cell order, NaN = cell left out), the mean and the population sd of the neighbourhood means, q x genes
        float64 each, and the cells per key, int64 (cna_gene_nbhd_corr).  timed=True: also (fill, step, moments) in
        milliseconds, the stream drained between the phases."""
        V = _f64(V)
        q, G = V.shape[0], self.expression_shape()['n_genes']
        r, mean, sd = (np.empty((q, G)) for _ in range(3))
        n_cells = np.zeros(q, dtype=np.int64)
        times = np.zeros(3) if timed else None
        check(self.lib.cna_gene_nbhd_corr(self.h, ptr(V), q, int(nsteps), ptr(r), ptr(mean), ptr(sd), ptr(n_cells), ptr(times)),
              'cna_gene_nbhd_corr')
        return (r, mean, sd, n_cells, times) if timed else (r, mean, sd, n_cells)

    def expr_to_bins(self, codes, n_bins, what):
        """Per-bin sums of the resident expression matrix (cna_expr_to_bins): `codes` int32 per cell in the caller's
        order, -1 = cell left out; `what` 0 sums x, 1 counts x > 0.  Returns (sums float64[n_bins, genes],
        counts int64[n_bins] of cells per bin)."""
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        info = self.expression_shape()
        if info['format'] != 'none' and codes.shape != (info['n_cells'],):
            raise ValueError('expr_to_bins: %d codes for %d resident cells' % (codes.size, info['n_cells']))
        n_bins = int(n_bins)
        sums = np.empty((max(n_bins, 0), info['n_genes']))
        counts = np.empty(max(n_bins, 0), dtype=np.int64)
        check(self.lib.cna_expr_to_bins(self.h, ptr(codes), n_bins, int(what), ptr(sums), ptr(counts)), 'cna_expr_to_bins')
        return sums, counts

    def gene_corr_by(self, V, codes, n_bins, want_within=True):
        """Pearson correlation of every gene of the resident expression matrix with every row of V (q x cells float64,
        caller's cell order, non-finite = cell left out of that key) inside every level of `codes` (int32 per cell, -1 =
        cell left out), and the pooled within-level correlation (cna_gene_corr_by).  Returns (r float64[q, n_bins, genes],
        within float64[q, genes] or None, n int64[q, n_bins]: cells of the level with a finite key)."""
        V = _f64(V)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        info = self.expression_shape()
        if info['format'] != 'none' and (V.ndim != 2 or codes.shape != (info['n_cells'],) or V.shape[1] != info['n_cells']):
            raise ValueError('gene_corr_by: keys %s and %d codes for %d resident cells'
                             % (V.shape, codes.size, info['n_cells']))
        q, n_bins = int(V.shape[0]), int(n_bins)
        r = np.empty((q, max(n_bins, 0), info['n_genes']))
        within = np.empty((q, info['n_genes'])) if want_within else None
        n = np.empty((q, max(n_bins, 0)), dtype=np.int64)
        check(self.lib.cna_gene_corr_by(self.h, ptr(V), q, ptr(codes), n_bins, ptr(r), None if within is None else ptr(within),
                                        ptr(n)), 'cna_gene_corr_by')
        return r, within, n

    def gene_ranksum_by(self, codes, n_levels, work_bytes=0):
        """Twice the rank sum of every level of `codes` (int32 per cell, -1 = cell left out) against all kept cells, for
        every gene of the resident expression matrix, midranks over the kept cells (cna_gene_ranksum_by).  `work_bytes`
        bounds the sort's keys of one tile of genes (0: the library's default).  Returns (rank2 int64[n_levels, genes],
        tie float64[genes]: sum of t^3 - t over the tie groups, n int64[n_levels]: cells per level, nan bool[genes]: a kept
        cell holds NaN and the gene's numbers mean nothing)."""
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        info = self.expression_shape()
        if info['format'] != 'none' and codes.shape != (info['n_cells'],):
            raise ValueError('gene_ranksum_by: %d codes for %d resident cells' % (codes.size, info['n_cells']))
        n_levels = int(n_levels)
        rank2 = np.empty((max(n_levels, 0), info['n_genes']), dtype=np.int64)
        tie = np.empty(info['n_genes'])
        n = np.empty(max(n_levels, 0), dtype=np.int64)
        nan = np.empty(info['n_genes'], dtype=np.uint8)
        check(self.lib.cna_gene_ranksum_by(self.h, ptr(codes), n_levels, int(work_bytes), ptr(rank2), ptr(tie), ptr(n),
                                           ptr(nan)), 'cna_gene_ranksum_by')
        return rank2, tie, n, nan.astype(bool)

    def gene_ranksum_pairs(self, codes, n_levels, pairs, work_bytes=0):
        """Level against level from one ranking of the kept cells of every gene (cna_gene_ranksum_pairs): `codes` int32
        per cell, -1 = cell left out, at most 64 levels; `pairs` int32[P, 2] of (level, versus), at most 2016.  Returns
        (u2 int64[P, genes]: twice the Mann-Whitney U of the level against the other one, tie float64[P, genes]: sum of
        t^3 - t over the tie groups of the two levels' cells, n int64[n_levels]: cells per level, nan bool[genes]: a kept
        cell of any level holds NaN and the gene's numbers mean nothing)."""
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        info = self.expression_shape()
        if info['format'] != 'none' and codes.shape != (info['n_cells'],):
            raise ValueError('gene_ranksum_pairs: %d codes for %d resident cells' % (codes.size, info['n_cells']))
        if pairs.ndim != 2 or pairs.shape[1] != 2:
            raise ValueError('gene_ranksum_pairs: pairs must be [P, 2], not %s' % (pairs.shape,))
        n_levels, n_pairs = int(n_levels), int(pairs.shape[0])
        u2 = np.empty((n_pairs, info['n_genes']), dtype=np.int64)
        tie = np.empty((n_pairs, info['n_genes']))
        n = np.empty(max(n_levels, 0), dtype=np.int64)
        nan = np.empty(info['n_genes'], dtype=np.uint8)
        check(self.lib.cna_gene_ranksum_pairs(self.h, ptr(codes), n_levels, ptr(pairs), n_pairs, int(work_bytes), ptr(u2),
                                              ptr(tie), ptr(n), ptr(nan)), 'cna_gene_ranksum_pairs')
        return u2, tie, n, nan.astype(bool)

    def gene_ranksum_within(self, codes, n_levels, blocks, n_blocks, w_num, w_tie, work_bytes=0):
        """Every level of `codes` against the rest inside every block of `blocks` (both int32 per cell, -1 = cell left out;
        at most 1024 levels and 255 blocks), ranked inside the block, the blocks folded with the caller's finite weights
        `w_num` float64[n_blocks] and `w_tie` float64[n_blocks, n_levels] (cna_gene_ranksum_within).  With D = 2 x the
        level's rank sum inside the block - n_sl (n_s + 1) and T the block's tie term, returns (d2 int64[n_levels, genes]:
        the sum of D over the blocks, num float64[n_levels, genes]: w_num[s] * D folded in block order, tiew
        float64[n_levels, genes]: w_tie[s, l] * T folded likewise, live int32[n_levels, genes]: blocks with 0 < n_sl < n_s
        in which the gene is not constant, n int64[n_blocks, n_levels]: kept cells, nan bool[genes]: a kept cell holds NaN
        and the gene's numbers mean nothing)."""
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        blocks = np.ascontiguousarray(blocks, dtype=np.int32)
        n_levels, n_blocks = int(n_levels), int(n_blocks)
        L, B = max(n_levels, 0), max(n_blocks, 0)
        w_num = _f64(w_num)
        w_tie = _f64(w_tie)
        info = self.expression_shape()
        if info['format'] != 'none' and (codes.shape != (info['n_cells'],) or blocks.shape != codes.shape):
            raise ValueError('gene_ranksum_within: %d level codes and %d block codes for %d resident cells'
                             % (codes.size, blocks.size, info['n_cells']))
        if w_num.shape != (B,) or w_tie.shape != (B, L):
            raise ValueError('gene_ranksum_within: weights %s and %s for %d blocks and %d levels'
                             % (w_num.shape, w_tie.shape, n_blocks, n_levels))
        G = info['n_genes']
        d2 = np.empty((L, G), dtype=np.int64)
        num, tiew = np.empty((L, G)), np.empty((L, G))
        live = np.empty((L, G), dtype=np.int32)
        n = np.empty((B, L), dtype=np.int64)
        nan = np.empty(G, dtype=np.uint8)
        check(self.lib.cna_gene_ranksum_within(self.h, ptr(codes), n_levels, ptr(blocks), n_blocks, ptr(w_num), ptr(w_tie),
                                               int(work_bytes), ptr(d2), ptr(num), ptr(tiew), ptr(live), ptr(n), ptr(nan)),
              'cna_gene_ranksum_within')
        return d2, num, tiew, live, n, nan.astype(bool)

    def gene_rank_corr(self, V, work_bytes=0):
        """The integers of Spearman's rank correlation of every gene of the resident expression matrix with every row of V
        (q x cells float64, caller's cell order, 1 <= q <= 16; a cell where any row is non-finite is left out of the whole
        call), midranks over the m kept cells (cna_gene_rank_corr).  `work_bytes` bounds the sort's entries of one tile of
        genes (0: the library's default).  Returns (s_lo uint64[q, genes], s_hi int64[q, genes]: S = sum of (2 r_gene - (m +
        1)) (2 r_key - (m + 1)) in 128-bit two's complement, tie_gene float64[genes], tie_key float64[q]: sum of t^3 - t over
        the tie groups, m int, nan bool[genes]: a kept cell holds NaN and the gene's numbers mean nothing)."""
        V = _f64(V)
        info = self.expression_shape()
        if info['format'] != 'none' and (V.ndim != 2 or V.shape[1] != info['n_cells']):
            raise ValueError('gene_rank_corr: keys %s for %d resident cells' % (V.shape, info['n_cells']))
        q = int(V.shape[0]) if V.ndim == 2 else 0
        s_lo = np.empty((max(q, 0), info['n_genes']), dtype=np.uint64)
        s_hi = np.empty((max(q, 0), info['n_genes']), dtype=np.int64)
        tie_gene = np.empty(info['n_genes'])
        tie_key = np.empty(max(q, 0))
        m = C.c_int64(0)
        nan = np.empty(info['n_genes'], dtype=np.uint8)
        check(self.lib.cna_gene_rank_corr(self.h, ptr(V), q, int(work_bytes), ptr(s_lo), ptr(s_hi), ptr(tie_gene), ptr(tie_key),
                                          C.byref(m), ptr(nan)), 'cna_gene_rank_corr')
        return s_lo, s_hi, tie_gene, tie_key, int(m.value), nan.astype(bool)

    def gene_rank_corr_by(self, V, codes, n_levels, work_bytes=0):
        """The integers of `gene_rank_corr` inside every level of `codes` (int32 per cell, -1 = cell left out, at most 255
        levels) from one sort of the matrix (cna_gene_rank_corr_by): level l is ranked over its cells where every row of V
        is finite, m[l] of them.  Returns (s_lo uint64[L, q, genes], s_hi int64[L, q, genes], tie_gene float64[L, genes],
        tie_key float64[L, q], m int64[L], nan bool[genes]: a kept cell of any level holds NaN and the gene's numbers mean
        nothing); level l's slices are what `gene_rank_corr` returns for V set to NaN outside the level."""
        V = _f64(V)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        info = self.expression_shape()
        if info['format'] != 'none' and (V.ndim != 2 or V.shape[1] != info['n_cells'] or codes.shape != (info['n_cells'],)):
            raise ValueError('gene_rank_corr_by: keys %s and %d codes for %d resident cells'
                             % (V.shape, codes.size, info['n_cells']))
        q = int(V.shape[0]) if V.ndim == 2 else 0
        L, G = max(int(n_levels), 0), info['n_genes']
        s_lo = np.empty((L, max(q, 0), G), dtype=np.uint64)
        s_hi = np.empty((L, max(q, 0), G), dtype=np.int64)
        tie_gene = np.empty((L, G))
        tie_key = np.empty((L, max(q, 0)))
        m = np.empty(L, dtype=np.int64)
        nan = np.empty(G, dtype=np.uint8)
        check(self.lib.cna_gene_rank_corr_by(self.h, ptr(V), q, ptr(codes), int(n_levels), int(work_bytes), ptr(s_lo), ptr(s_hi),
                                             ptr(tie_gene), ptr(tie_key), ptr(m), ptr(nan)), 'cna_gene_rank_corr_by')
        return s_lo, s_hi, tie_gene, tie_key, m, nan.astype(bool)

    def _x_columns_args(self, xrow, Z, who):
        """(xrow int64, Z float64 C-contiguous, q, expression_shape()) of the entries that form per-cell columns from the working matrix X: one
        rank with a replicated view, one xrow per resident cell, one row of Z per column with one entry per sample of X."""
        if self.nranks != 1 or self.view_local:
            raise NotImplementedError('%s needs every row of X on this rank (one rank, replicated view)' % who)
        xrow = np.ascontiguousarray(xrow, dtype=np.int64)
        Z = _f64(Z)
        info = self.expression_shape()
        if info['format'] != 'none':
            cols = self.matrix_shape(MAT_X)[1]
            if xrow.shape != (info['n_cells'],) or Z.ndim != 2 or Z.shape[1] != cols:
                raise ValueError('%s: xrow %s and Z %s for %d resident cells and %d samples of X'
                                 % (who, xrow.shape, Z.shape, info['n_cells'], cols))
        return xrow, Z, (int(Z.shape[0]) if Z.ndim == 2 else 0), info

    def x_columns(self, xrow, Z):
        """float64[q, cells]: out[j, i] = sum over the samples s, ascending, of X[xrow[i], s] * Z[j, s] -- each product
        rounded, then added -- for the cells with a row in the working matrix X (`x_row_of_cells`), NaN where xrow[i] is -1
        (cna_x_columns).  Z: q x samples, 1 <= q <= 4096.  One rank, replicated view.  No memo."""
        xrow, Z, q, info = self._x_columns_args(xrow, Z, 'x_columns')
        out = np.empty((max(q, 0), len(xrow)))
        check(self.lib.cna_x_columns(self.h, ptr(xrow), len(xrow), ptr(Z), q, ptr(out)), 'cna_x_columns')
        return out

    def _rank_corr_outputs(self, q, G):
        return (np.empty((max(q, 0), G), dtype=np.uint64), np.empty((max(q, 0), G), dtype=np.int64), np.empty(G),
                np.empty(max(q, 0)), C.c_int64(0), np.empty(G, dtype=np.uint8))

    def gene_rank_corr_x(self, xrow, Z, work_bytes=0):
        """`gene_rank_corr`'s integers for the q columns `x_columns(xrow, Z)` forms, 1 <= q <= 4096, from one sort of the
        resident matrix whatever q is (cna_gene_rank_corr_x): the columns are formed and ranked on the device in groups
        of 16.  The kept cells are those with xrow[i] >= 0; a formed value that is not finite is refused.  Returns
        `gene_rank_corr`'s tuple.  One rank, replicated view.  No memo: the columns differ with every phenotype."""
        xrow, Z, q, info = self._x_columns_args(xrow, Z, 'gene_rank_corr_x')
        s_lo, s_hi, tie_gene, tie_key, m, nan = self._rank_corr_outputs(q, info['n_genes'])
        check(self.lib.cna_gene_rank_corr_x(self.h, ptr(xrow), len(xrow), ptr(Z), q, int(work_bytes), ptr(s_lo), ptr(s_hi),
                                            ptr(tie_gene), ptr(tie_key), C.byref(m), ptr(nan)), 'cna_gene_rank_corr_x')
        return s_lo, s_hi, tie_gene, tie_key, int(m.value), nan.astype(bool)

    def gene_rank_corr_x_by(self, xrow, Z, codes, n_levels, work_bytes=0):
        """`gene_rank_corr_x` inside every level of `codes` (int32 per cell, -1 = cell left out, at most 255 levels) from
        one sort of the resident matrix per library call (cna_gene_rank_corr_x_by): level l is ranked over its cells with
        xrow[i] >= 0, m[l] of them.  Returns (s_lo uint64[L, q, genes], s_hi int64[L, q, genes], tie_gene float64[L, genes],
        tie_key float64[L, q], m int64[L], nan bool[genes]); level l's slices are what `gene_rank_corr_x` returns for xrow
        set to -1 outside the level, and every group of 16 columns what `gene_rank_corr_by` returns for those rows of
        `x_columns(xrow, Z)`.  The integers take 16 L q genes bytes: the rows of Z go in chunks of whole groups of 16 whose
        results stay within RANK_X_BY_HOST_BYTES (one group at least) and the chunks are concatenated -- a group's
        integers depend on xrow, codes and its own 16 rows alone, so the chunking changes no bit.  One rank, replicated
        view.  No memo."""
        xrow, Z, q, info = self._x_columns_args(xrow, Z, 'gene_rank_corr_x_by')
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if info['format'] != 'none' and codes.shape != xrow.shape:
            raise ValueError('gene_rank_corr_x_by: %d codes for %d resident cells' % (codes.size, info['n_cells']))
        L, G = max(int(n_levels), 0), info['n_genes']
        s_lo = np.empty((L, max(q, 0), G), dtype=np.uint64)
        s_hi = np.empty((L, max(q, 0), G), dtype=np.int64)
        tie_gene, tie_key = np.empty((L, G)), np.empty((L, max(q, 0)))
        m, nan = np.empty(L, dtype=np.int64), np.empty(G, dtype=np.uint8)

        def call(Zc, lo, hi, tk):
            check(self.lib.cna_gene_rank_corr_x_by(self.h, ptr(xrow), len(xrow), ptr(Zc), int(Zc.shape[0]) if Zc.ndim == 2 else 0,
                                                   ptr(codes), int(n_levels), int(work_bytes), ptr(lo), ptr(hi), ptr(tie_gene),
                                                   ptr(tk), ptr(m), ptr(nan)), 'cna_gene_rank_corr_x_by')

        step = 16 * max(1, int(RANK_X_BY_HOST_BYTES) // max(1, 16 * 16 * L * G))      # columns of one call
        if q <= step or q > 4096:
            call(Z, s_lo, s_hi, tie_key)                       # (and every q the library refuses: the refusal is the library's)
        else:
            for k0 in range(0, q, step):                       # tie_gene, m and nan are every chunk's alike
                cols = min(step, q - k0)
                lo, hi = np.empty((L, cols, G), dtype=np.uint64), np.empty((L, cols, G), dtype=np.int64)
                tk = np.empty((L, cols))
                call(np.ascontiguousarray(Z[k0:k0 + cols]), lo, hi, tk)
                s_lo[:, k0:k0 + cols], s_hi[:, k0:k0 + cols], tie_key[:, k0:k0 + cols] = lo, hi, tk
        return s_lo, s_hi, tie_gene, tie_key, m, nan.astype(bool)

    def gene_rank_corr_wide(self, V, work_bytes=0):
        """`gene_rank_corr` for 1 <= q <= 4096 rows of V (q x cells float64) from one sort of the resident matrix
        (cna_gene_rank_corr_wide): the kept cells are those where every one of the q rows is finite, one set per call.
        Returns `gene_rank_corr`'s tuple; every group of 16 rows holds what `gene_rank_corr` returns for those rows under
        that kept set.  One rank, replicated view."""
        if self.nranks != 1 or self.view_local:
            raise NotImplementedError('gene_rank_corr_wide needs every cell on this rank (one rank, replicated view)')
        V = _f64(V)
        info = self.expression_shape()
        if info['format'] != 'none' and (V.ndim != 2 or V.shape[1] != info['n_cells']):
            raise ValueError('gene_rank_corr_wide: keys %s for %d resident cells' % (V.shape, info['n_cells']))
        q = int(V.shape[0]) if V.ndim == 2 else 0
        s_lo, s_hi, tie_gene, tie_key, m, nan = self._rank_corr_outputs(q, info['n_genes'])
        check(self.lib.cna_gene_rank_corr_wide(self.h, ptr(V), q, int(work_bytes), ptr(s_lo), ptr(s_hi), ptr(tie_gene),
                                               ptr(tie_key), C.byref(m), ptr(nan)), 'cna_gene_rank_corr_wide')
        return s_lo, s_hi, tie_gene, tie_key, int(m.value), nan.astype(bool)

    BW_KINDS =('scott', 'silverman', 'constant')

    def coef_strata(self, v, fdr, codes, n_bins, fdr_thresh, points, bw_kind='scott', bw_value=0.0):
        """Per-bin statistics and kernel densities of a per-cell column (cna_coef_strata): `v` float64 per cell in the
        caller's order (NaN / inf = no value), `fdr` the same or None, `codes` int32 per cell, -1 = cell left out;
        `bw_kind` one of 'scott', 'silverman', 'constant' (`bw_value` is then the bandwidth factor).  Returns a dict:
        n, n_kept, n_pos, n_neg int64[n_bins]; mean, ssd, min, median, max float64[n_bins]; vals float64[n_bins, points].
        Needs no graph and no resident expression matrix; `drop_expression` frees its device buffers."""
        v = np.ascontiguousarray(v, dtype=np.float64)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if fdr is not None:
            fdr = np.ascontiguousarray(fdr, dtype=np.float64)
        if v.ndim != 1 or codes.shape != v.shape or (fdr is not None and fdr.shape != v.shape):
            raise ValueError('coef_strata: v, fdr and codes must be 1-D and of one length')
        n_bins, points = int(n_bins), int(points)
        nb, npts = max(n_bins, 0), max(points, 0)
        out = {k: np.empty(nb, dtype=np.int64) for k in ('n', 'n_kept', 'n_pos', 'n_neg')}
        out.update({k: np.empty(nb) for k in ('mean', 'ssd', 'min', 'median', 'max')})
        out['vals'] = np.empty((nb, npts))
        check(self.lib.cna_coef_strata(self.h, ptr(v), None if fdr is None else ptr(fdr), ptr(codes), v.size, n_bins, points,
                                       self.BW_KINDS.index(bw_kind), float(bw_value), float(fdr_thresh),
                                       *[ptr(out[k]) for k in ('n', 'n_kept', 'n_pos', 'n_neg', 'mean', 'ssd', 'min', 'median',
                                                               'max', 'vals')]), 'cna_coef_strata')
        return out

    def coef_raster(self, xy, V, FDR, has_fdr, fdr_thresh, extent, width, height, radius=0):
        """Per-pixel counts, sums and extremes of per-cell columns on a 2-D embedding (cna_coef_raster): `xy` cells x 2
        float64, `V` q x cells float64 (NaN / inf = the cell does not pass), `FDR` the same shape or None, `has_fdr` one
        flag per key (a key without one passes every finite value), `extent` (x0, x1, y0, y1) or None = the finite cells'
        min and max, found on the device.  Returns a dict: extent (4-tuple), n int64[H, W], n_outside int, n_pass
        int64[q, H, W], sum, top, bottom float64[q, H, W], covered bool[H, W], absmax float64[q]; with radius > 0 top,
        bottom and covered are dilated by the disc.  ValueError when no cell has finite coordinates.  Needs no graph and no
        resident expression matrix; `drop_expression` frees its device buffers."""
        xy = np.ascontiguousarray(xy, dtype=np.float64)
        V = _f64(V)
        has_fdr = np.ascontiguousarray(has_fdr, dtype=np.int32)
        if FDR is not None:
            FDR = _f64(FDR)
        if xy.ndim != 2 or xy.shape[1] != 2 or V.ndim != 2 or V.shape[1] != xy.shape[0] or has_fdr.shape != (V.shape[0],) \
                or (FDR is not None and FDR.shape != V.shape) or (FDR is None and has_fdr.any()):
            raise ValueError('coef_raster: xy is cells x 2, V and FDR are keys x cells, has_fdr has one flag per key')
        q, W, H = int(V.shape[0]), int(width), int(height)
        # sizes the library refuses get one-pixel outputs: it writes nothing then
        Wp, Hp = (W, H) if 1 <= W <= 4096 and 1 <= H <= 4096 and q * W * H <= 2 ** 22 else (1, 1)
        ext = np.zeros(4) if extent is None else np.array(extent, dtype=np.float64).reshape(4)
        out = {'n': np.empty((Hp, Wp), dtype=np.int64), 'n_pass': np.empty((q, Hp, Wp), dtype=np.int64)}
        out.update({k: np.empty((q, Hp, Wp)) for k in ('sum', 'top', 'bottom')})
        covered = np.empty((Hp, Wp), dtype=np.uint8)
        absmax, n_outside = np.empty(q), np.zeros(1, dtype=np.int64)
        check(self.lib.cna_coef_raster(self.h, ptr(xy), ptr(V), ptr(FDR), ptr(has_fdr), q, xy.shape[0], float(fdr_thresh),
                                       ptr(ext), int(extent is None), W, H, int(radius), ptr(out['n']), ptr(n_outside),
                                       ptr(out['n_pass']), ptr(out['sum']), ptr(out['top']), ptr(out['bottom']), ptr(covered),
                                       ptr(absmax)), 'cna_coef_raster')
        if np.isnan(ext).any():
            raise ValueError('coef_raster: no cell has finite coordinates, so there is no extent')
        out.update(extent=tuple(float(e) for e in ext), n_outside=int(n_outside[0]), covered=covered.view(np.bool_), absmax=absmax)
        return out

    def graph_components(self, codes, min_cells=1, n_classes=None):
        """Connected components of the resident graph inside classes of cells, on the device (cna_graph_components_find /
        _list / _label): `codes` int32 per cell in the CALLER's order, a class >= 0 or -1 for none (`n_classes` defaults to
        the largest code + 1).  Two classed cells share a component when a chain of stored entries joins them, read in
        either direction, through cells of their class; an entry is an edge whatever its value, a stored zero included.
        The device reads the codes and writes the labels through its own cell order, so nothing per cell is permuted here.
        Returns (comp, list, n_components_total): `comp` int32 per cell in the caller's order, the index of the cell's
        component in `list` or -1; `list` a dict of arrays over the components with at least `min_cells` cells -- 'class'
        int32, 'size' int64, 'first' int64, the smallest caller cell index -- sorted by class, then size descending, then
        'first'; `n_components_total` int64 per class, before that filter.  `self.sweeps` holds the hook / flatten / check
        rounds the call took (1 to 32).  The graph is the one `ensure_graph` left; NAM and X stay as they are.  One rank,
        replicated view."""
        if self.nranks != 1 or self.view_local:
            raise NotImplementedError('graph_components needs every row of the graph on this rank (one rank, replicated view)')
        if self._graph_key is None:
            raise ValueError('graph_components: no graph is resident (ensure_graph first)')
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if codes.shape != (int(self.n),):
            raise ValueError('graph_components: %s codes for %d cells' % (codes.shape, int(self.n)))
        if n_classes is None:
            n_classes = int(codes.max(initial=-1)) + 1
        n_classes = int(n_classes)
        totals = np.zeros(max(n_classes, 1), dtype=np.int64)
        kept, sweeps = C.c_int64(0), C.c_int(0)
        check(self.lib.cna_graph_components_find(self.h, ptr(codes), codes.size, max(n_classes, 1), int(max(min_cells, 1)),
                                                 C.byref(kept), ptr(totals), C.byref(sweeps)), 'cna_graph_components_find')
        self.sweeps = int(sweeps.value)
        K = int(kept.value)
        cls, size, first = (np.empty(K, dtype=np.int32) for _ in range(3))
        check(self.lib.cna_graph_components_list(self.h, K, ptr(cls), ptr(size), ptr(first)), 'cna_graph_components_list')
        order = np.lexsort((first, -size.astype(np.int64), cls))        # the list arrives in no fixed order
        rank = np.empty(K, dtype=np.int32)
        rank[order] = np.arange(K, dtype=np.int32)
        comp = np.empty(codes.size, dtype=np.int32)
        check(self.lib.cna_graph_components_label(self.h, ptr(rank), K, ptr(comp), codes.size), 'cna_graph_components_label')
        lst = {'class': cls[order], 'size': size[order].astype(np.int64), 'first': first[order].astype(np.int64)}
        return comp, lst, totals[:n_classes]

    def matrix_to_bins(self, which, codes, W=None, n_bins=None):
        """Weighted per-bin sums over the rows of the resident NAM (MAT_NAM) or of the working matrix X (MAT_X), on the
        device (cna_matrix_to_bins): `codes` int32 per cell in the CALLER's order, -1 = cell left out; `W` q x cells
        float64 in the caller's order (a weight that is zero or not finite leaves the cell out of that column) or None:
        every weight 1; `n_bins` defaults to the largest code + 1.  The cells are mapped to the matrix' rows here: the
        device's cell order for the NAM, `x_row_of_cells()` for an X that is a selection (a cell it dropped contributes
        nothing), the identity for an X from `upload_x` (one code per row).  Returns (sums float64[max(q, 1), n_bins,
        n_cols], n int64[max(q, 1), n_bins]: the contributing cells).  One rank, replicated view."""
        if self.nranks != 1 or self.view_local:
            raise NotImplementedError('matrix_to_bins needs every row of the matrix on this rank (one rank, replicated view)')
        if which not in (MAT_NAM, MAT_X):
            raise ValueError('matrix_to_bins: which is MAT_NAM or MAT_X')
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if W is not None:
            W = _f64(W)
        selection = which == MAT_X and self._x_is_selection
        cells = int(self.x_rows_total) if which == MAT_X and not selection else int(self.n)
        if codes.shape != (cells,):
            raise ValueError('matrix_to_bins: %s codes for %d cells' % (codes.shape, cells))
        if W is not None and (W.ndim != 2 or W.shape[1] != cells):
            raise ValueError('matrix_to_bins: weights %s for %d cells (q x cells)' % (W.shape, cells))
        if n_bins is None:
            n_bins = max(int(codes.max(initial=-1)) + 1, 1)
        if which == MAT_NAM:
            if self.perm is not None:
                codes = np.ascontiguousarray(codes[self.perm])
                W = None if W is None else np.ascontiguousarray(W[:, self.perm])
        elif selection:
            codes, W = _rows_of_x(self.x_row_of_cells(), int(self.x_rows_total), codes, W)
        return self.matrix_rows_to_bins(which, codes, W, n_bins)

    def matrix_rows_to_bins(self, which, codes, W, n_bins):
        """cna_matrix_to_bins as it is: `codes` and the columns of `W` (or None) are per LOCAL ROW of the matrix."""
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        W = None if W is None else _f64(W)
        q = 0 if W is None else int(W.shape[0])
        n_bins = int(n_bins)
        n_cols = self.matrix_shape(which)[1]
        sums = np.empty((max(q, 1), max(n_bins, 0), n_cols))
        n = np.empty((max(q, 1), max(n_bins, 0)), dtype=np.int64)
        check(self.lib.cna_matrix_to_bins(self.h, int(which), ptr(codes), ptr(W), q, codes.size, n_bins, ptr(sums), ptr(n)),
              'cna_matrix_to_bins')
        return sums, n

    def enrichment_extremes(self, R, set_ptr, set_genes, weight):
        """The running-sum extremes of gene set enrichment for every set under every row of `R` (n_cols x genes float64,
        the observed correlations first, then one row per null column; a non-finite entry leaves the gene out of that
        row), on the device (cna_enrichment_extremes): `set_ptr` n_sets + 1 offsets into `set_genes`, the members' gene
        indices, ascending and distinct inside a set; `weight` 0, 1 or 2, the exponent of |r|.  Returns (up float64[n_cols,
        n_sets], down likewise, size int32[n_cols, n_sets]: the set's valid members, valid int32[n_cols]: the row's valid
        genes); up and down are NaN where the set has no valid member, every valid gene, or no weight.  Needs no graph
        and no resident expression matrix; `drop_expression` frees its device buffers."""
        R = _f64(R)
        set_ptr = np.ascontiguousarray(set_ptr, dtype=np.int64)
        set_genes = np.ascontiguousarray(set_genes, dtype=np.int32)
        if R.ndim != 2 or set_ptr.ndim != 1 or set_genes.ndim != 1 or len(set_ptr) < 2 or set_ptr[-1] != len(set_genes):
            raise ValueError('enrichment_extremes: R is n_cols x genes, set_ptr holds n_sets + 1 offsets that end at len(set_genes)')
        n_cols, n_genes = R.shape
        n_sets = len(set_ptr) - 1
        up, down = np.empty((n_cols, n_sets)), np.empty((n_cols, n_sets))
        size = np.empty((n_cols, n_sets), dtype=np.int32)
        valid = np.empty(n_cols, dtype=np.int32)
        if not len(set_genes):
            set_genes = np.zeros(1, dtype=np.int32)         # a pointer the library can take; no offset reaches it
        check(self.lib.cna_enrichment_extremes(self.h, ptr(R), n_cols, n_genes, ptr(set_ptr), ptr(set_genes), n_sets, int(weight),
                                               ptr(up), ptr(down), ptr(size), ptr(valid)), 'cna_enrichment_extremes')
        return up, down, size, valid

    def x_generation(self):
        """How often the library has voided the working matrix X so far (cna_x_generation: every producer of X and every
        transition above it, in place or not)."""
        g = C.c_int64(0)
        check(self.lib.cna_x_generation(self.h, C.byref(g)), 'cna_x_generation')
        return g.value

    def expr_cross(self, content=None, xrow=None):
        """(W, rho, sx, sxx, m) of the resident expression matrix E against the working matrix X (cna_expr_cross):
        W = E_K^T X (genes x samples float64), rho the column sums of X, sx / sxx the per-gene sums of x and x^2, all over
        the m cells that have a row in X (`x_row_of_cells`: the caller's order against the device order and the
        selection).  One rank, replicated view.

        Memo: the result is kept under (uploads of the expression matrix, x_epoch, the library's X generation) -- every
        transition that voids what is derived from X moves the last of them (csrc/c_api.hip:void_x) -- and a call under
        the same key launches nothing (`cross_launches` counts the launches).  `content`: the caller's word for what X
        was made from (cna.tl.gene_test: the NAM's signature, the kept cells, the samples, the projector and the Gram
        matrix' bits); a further analysis rebuilds X, so the key moves, but under an equal `content` the X is the same
        and the memo is carried over to the new key instead of being taken again.  (x_epoch alone cannot serve a second
        phenotype: every association selects and residualises anew, so X is rebuilt -- to the same bits -- and the epoch
        moves with every call.)  `cross_extra()` is a dict that lives and dies with the memo, for what else a caller
        derives from the same E and the same cells.  `xrow`: an explicit map instead of `x_row_of_cells()`; such a call
        neither reads nor writes the memo."""
        if self.nranks != 1 or self.view_local:
            raise NotImplementedError('expr_cross needs every row of X on this rank (one rank, replicated view)')
        info = self.expression_shape()
        key = _x_key(self, info)
        memo = None if xrow is not None else _memo_lookup(self._cross_memo, key, content, None)
        if memo is not None:
            return memo.result
        g = info['n_genes']
        cols = self.matrix_shape(MAT_X)[1] if info['format'] != 'none' else 0
        explicit = xrow is not None
        xrow = np.ascontiguousarray(xrow if explicit else self.x_row_of_cells(), dtype=np.int64)
        W, rho = np.empty((g, cols)), np.empty(cols)
        sx, sxx = np.empty(g), np.empty(g)
        m = C.c_int64(0)
        self.cross_launches += 1
        check(self.lib.cna_expr_cross(self.h, ptr(xrow), len(xrow), ptr(W), ptr(rho), ptr(sx), ptr(sxx), C.byref(m)),
              'cna_expr_cross')
        out = (W, rho, sx, sxx, int(m.value))
        if not explicit:
            self._cross_memo = _memo_store(key, content, None, out)
        return out

    def cross_extra(self):
        """The dict that goes with the current expr_cross memo (empty after every launch, gone with the memo)."""
        return {} if self._cross_memo is None else self._cross_memo.extra

    CROSS_BY_HOST_BYTES = 1 << 30      # the whole W of expr_cross_by that is taken in one call and kept

    def expr_cross_by_raw(self, xrow, codes, n_bins, bin0=0, nb=None):
        """(W float64[nb, genes, samples], sx, sxx float64[nb, genes], m int64[nb]) for the levels [bin0, bin0 + nb) of
        `codes` (int32 per cell, -1 = cell left out), `xrow` the row of X of every cell.  A dense resident matrix:
        cna_expr_cross_by, one pass for all levels.  Gene-major lists: one cna_expr_cross per level with xrow masked to
        that level -- the one-pass kernel for that form lost its measurement at 1M cells x 100 samples
        (profiles/kbench_gene_test_strata.txt) and is not in the library; the codes are checked here, and a refusal is a
        CnaHipError in either form."""
        xrow = np.ascontiguousarray(xrow, dtype=np.int64)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if xrow.ndim != 1 or codes.shape != xrow.shape:
            raise ValueError('expr_cross_by: xrow and codes must be 1-D and of one length')
        n_bins, bin0 = int(n_bins), int(bin0)
        nb = n_bins - bin0 if nb is None else int(nb)
        info = self.expression_shape()
        g = info['n_genes']
        cols = self.matrix_shape(MAT_X)[1] if info['format'] != 'none' else 0
        k = max(nb, 0)
        W, sx, sxx, m = np.empty((k, g, cols)), np.empty((k, g)), np.empty((k, g)), np.empty(k, dtype=np.int64)
        if info['format'] == 'gene-major':
            # the checks cna_expr_cross_by makes, under the error type it raises through check()
            if not 1 <= n_bins <= 1024 or bin0 < 0 or nb < 1 or bin0 + nb > n_bins:
                raise _ffi.CnaHipError('expr_cross_by failed: 1 <= n_bins <= 1024 and the levels [bin0, bin0 + nb) must lie in '
                                       '[0, n_bins), nb >= 1')
            if len(codes) and (codes.min() < -1 or codes.max() >= n_bins):
                raise _ffi.CnaHipError('expr_cross_by failed: a code lies outside [-1, n_bins)')
            for l in range(nb):
                W[l], _, sx[l], sxx[l], m[l] = self.expr_cross(xrow=np.where(codes == bin0 + l, xrow, -1))
            return W, sx, sxx, m
        check(self.lib.cna_expr_cross_by(self.h, ptr(xrow), ptr(codes), len(xrow), n_bins, bin0, nb, ptr(W), ptr(sx), ptr(sxx),
                                         ptr(m)), 'cna_expr_cross_by')
        return W, sx, sxx, m

    def gram_by(self, xrow, codes, n_bins):
        """cna_gram_by: (Gamma float64[n_bins, samples, samples], m int64[n_bins]), Gamma[l] = X_l^T X_l over the rows
        xrow[i] >= 0 of the working matrix X of the cells with codes[i] == l.  Needs no resident expression matrix."""
        xrow = np.ascontiguousarray(xrow, dtype=np.int64)
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        if xrow.ndim != 1 or codes.shape != xrow.shape:
            raise ValueError('gram_by: xrow and codes must be 1-D and of one length')
        n_bins = int(n_bins)
        cols = self.matrix_shape(MAT_X)[1]
        k = max(n_bins, 0)
        Gm, m = np.empty((k, cols, cols)), np.empty(k, dtype=np.int64)
        check(self.lib.cna_gram_by(self.h, ptr(xrow), ptr(codes), len(xrow), n_bins, ptr(Gm), ptr(m)), 'cna_gram_by')
        return Gm, m

    def expr_cross_by(self, codes, n_bins, bins=None, content=None, xrow=None):
        """`expr_cross` inside every level of a clustering: (W, rho, sx, sxx, m, Gamma) for the levels `bins` (default: all
        `n_bins`) of `codes` (int32 per cell in the caller's order, -1 = cell left out), over the cells of each level
        that have a row in X: W float64[levels, genes, samples] = E_l^T X_l (`expr_cross_by_raw`), rho float64[levels,
        samples] the column sums of X_l (`matrix_rows_to_bins(MAT_X, ...)`), sx / sxx float64[levels, genes], m
        int64[levels] the cells, Gamma float64[levels, samples, samples] = X_l^T X_l (cna_gram_by).  One rank, replicated
        view.

        Memo: beside `expr_cross`'s and under the same key (uploads of the expression matrix, x_epoch, the library's X
        generation) plus a digest of the codes and n_bins; carried over to a new key under an equal `content`, as there;
        void wherever that memo is.  `cross_by_launches` counts the calls that went to the device, `cross_by_extra()` is
        the dict that lives and dies with the memo.  An explicit `xrow` neither reads nor writes the memo.

        When W for all n_bins levels (levels x genes x samples x 8 bytes) or Gamma does not fit 1 GiB of host memory, the
        method works in groups of levels -- the requested ones only -- and keeps no memo: every such call passes over the
        expression matrix once per group."""
        if self.nranks != 1 or self.view_local:
            raise NotImplementedError('expr_cross_by needs every row of X on this rank (one rank, replicated view)')
        codes = np.ascontiguousarray(codes, dtype=np.int32)
        n_bins = int(n_bins)
        info = self.expression_shape()
        resident = info['format'] != 'none'
        key = _x_key(self, info)
        tag = (array_digest(codes), n_bins)
        sel = None if bins is None else np.asarray(bins, dtype=np.int64).reshape(-1)
        if sel is not None and len(sel) and (sel.min() < 0 or sel.max() >= n_bins):
            raise ValueError('expr_cross_by: bins must lie in [0, n_bins)')

        def pick(out):
            return out if sel is None else tuple(a[sel] for a in out)
        memo = None if xrow is not None else _memo_lookup(self._cross_by_memo, key, content, tag)
        if memo is not None:
            return pick(memo.result)
        g = info['n_genes']
        cols = self.matrix_shape(MAT_X)[1] if resident else 0
        explicit = xrow is not None
        xrow = np.ascontiguousarray(xrow if explicit else self.x_row_of_cells(), dtype=np.int64)

        def take(cd, k):
            """the k levels of the codes cd, W and Gamma each in groups that fit"""
            step = max(1, self.CROSS_BY_HOST_BYTES // max(1, 8 * g * cols))
            parts = [self.expr_cross_by_raw(xrow, cd, k, b0, min(step, k - b0)) for b0 in range(0, k, step)]
            W, sx, sxx, m = (np.concatenate([p_[j] for p_ in parts]) if len(parts) > 1 else parts[0][j] for j in range(4))
            gstep = max(1, self.CROSS_BY_HOST_BYTES // max(1, 8 * cols * cols))
            grams = [self.gram_by(xrow, np.where((cd >= b0) & (cd < b0 + gstep), cd - b0, -1), min(gstep, k - b0))[0]
                     for b0 in range(0, k, gstep)]
            Gamma = np.concatenate(grams) if len(grams) > 1 else grams[0]
            rho = self.matrix_rows_to_bins(MAT_X, _rows_of_x(xrow, int(self.x_rows_total), cd)[0], None, k)[0][0]
            self.cross_by_launches += 1                               # counted once nothing has been refused
            return W, rho, sx, sxx, m, Gamma
        fits = 8 * n_bins * g * cols <= self.CROSS_BY_HOST_BYTES and 8 * n_bins * cols * cols <= self.CROSS_BY_HOST_BYTES
        if not fits and n_bins >= 1:
            want = np.arange(n_bins) if sel is None else sel
            lut = np.full(n_bins + 1, -1, dtype=np.int32)            # the last entry serves the code -1
            lut[want] = np.arange(len(want), dtype=np.int32)
            ok = (codes >= -1) & (codes < n_bins)
            self._cross_by_memo = None
            return take(np.where(ok, lut[np.where(ok, codes, -1)], codes).astype(np.int32), len(want))
        out = take(codes, n_bins)
        if not explicit:
            self._cross_by_memo = _memo_store(key, content, tag, out)
        return pick(out)

    def cross_by_extra(self):
        """The dict that goes with the current expr_cross_by memo (empty after every launch, gone with the memo)."""
        return {} if self._cross_by_memo is None else self._cross_by_memo.extra

    # ---------------------------------------------------------------- synthetic inputs
    def knn_graph(self, X, k):
        """scanpy-like connectivities of the points X (n x d, d <= 64) built on the device
        (cna_knn_graph): CSR float32 / int32, sorted indices.  Input generator for benchmarks."""
        X = np.ascontiguousarray(X, dtype=np.float32)
        n, d = X.shape
        cap = 2 * n * (k - 1)
        indptr = np.empty(n + 1, dtype=np.int64)
        indices = np.empty(cap, dtype=np.int32)
        data = np.empty(cap, dtype=np.float32)
        nnz = C.c_int64(0)
        check(self.lib.cna_knn_graph(self.h, ptr(X), n, d, int(k), ptr(indptr), ptr(indices), ptr(data), C.byref(nnz)),
              'cna_knn_graph')
        m = nnz.value
        A = sp.csr_matrix((data[:m].copy(), indices[:m].copy(), indptr.astype(np.int32 if m < 2 ** 31 else np.int64)),
                          shape=(n, n))
        A.has_sorted_indices = True
        return A

    # ---------------------------------------------------------------- measurement
    def prof_enable(self, on=True, walk_only=False):
        """HIP-event timing of the kernel groups (include/cna_hip.h: cna_prof_enable); walk_only: the walk kernels and the
        communication spans only."""
        check(self.lib.cna_prof_enable(self.h, (2 if walk_only else 1) if on else 0), 'cna_prof_enable')

    def prof_reset(self):
        check(self.lib.cna_prof_reset(self.h), 'cna_prof_reset')

    def prof(self):
        """{kernel name: (total ms, launches)} for kernels launched while profiling was on."""
        out = {}
        for k, name in enumerate(_ffi.KERNELS + _ffi.KERNELS_RANK_CORR):
            ms, n = C.c_double(0.0), C.c_int64(0)
            check(self.lib.cna_prof_get(self.h, k, C.byref(ms), C.byref(n)), 'cna_prof_get')
            if n.value:
                out[name] = (ms.value, n.value)
        return out


_check_pool = None


_REORDER_ASYNC = os.environ.get('CNA_REORDER_ASYNC', '1') not in ('0', 'off', 'no')
_REORDER_ASYNC_CELLS = 100000
_reorder_workers = None


def _reorder_pool():
    global _reorder_workers
    if _reorder_workers is None:
        from concurrent.futures import ThreadPoolExecutor
        _reorder_workers = ThreadPoolExecutor(max_workers=1, thread_name_prefix='cna-order')
    return _reorder_workers


def _checker():
    """One thread for deferred graph checks (the hash itself runs on the library's own threads)."""
    global _check_pool
    if _check_pool is None:
        from concurrent.futures import ThreadPoolExecutor
        _check_pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix='cna-graph-check')
    return _check_pool


def _forget_pools():
    """In a forked child the worker threads of these pools do not exist; the next user makes new ones."""
    global _reorder_workers, _check_pool
    _reorder_workers = _check_pool = None


if hasattr(os, 'register_at_fork'):
    os.register_at_fork(after_in_child=_forget_pools)

_default = None


def get_engine():
    """The process-wide engine (created on first use; one GPU per process)."""
    global _default
    if _default is None:
        from . import dist
        cfg = dist.current()
        _default = Engine(device=cfg.get('device'), rank=cfg.get('rank', 0), nranks=cfg.get('nranks', 1),
                          unique_id=cfg.get('unique_id'), shm=cfg.get('shm'))
    return _default


def set_engine(engine):
    global _default
    _default = engine
