"""Client-major delta slab: the HBM layout of K client deltas for one round.

The reference keeps one pytree per client (examples/fed_avg.py:72-76 holds all K
at once in a Python list). On MI355X the fold is fastest when every client's
delta is one contiguous row of a single allocation::

    slab[K, P]   row k = client k's leaves back to back, jax flatten order
                 (dict keys sorted), row stride padded to 16 bytes

so one launch of the dense kernel streams K*P elements with 1 KiB coalesced
wave loads and writes one P-element result. 288 GB of HBM holds e.g. 1024
clients x 4 M f32 params (17 GB) or 1024 x 125 M bf16 (256 GB) per GPU.

``client(k)`` returns a pytree of views into row k, so client training (or an
H2D copy of a host-resident delta) writes straight into the slab; those views
also work with :func:`fedjax_amd.tree_util.tree_mean` (pytree path).
"""

from __future__ import annotations

from typing import Optional, Sequence

import numpy as np
import torch

from fedjax_amd import _lib, kernels, pytree, tree_util
from fedjax_amd.typing import PyTree


class ClientDeltaSlab:
    """K client deltas sharing one pytree structure, as one [K, P] device tensor."""

    def __init__(self, template: PyTree, num_clients: int, *, dtype: torch.dtype = torch.float32,
                 device: Optional[torch.device] = None):
        if dtype not in (torch.float32, torch.bfloat16):
            raise TypeError("slab dtype must be float32 or bfloat16")
        leaves, self.treedef = pytree.flatten(template)
        self.shapes = [tuple(tree_util._to_tensor(x).shape) for x in leaves]
        self.sizes = [int(np.prod(s, dtype=np.int64)) for s in self.shapes]
        self.offsets = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.num_params = int(self.offsets[-1])
        self.num_clients = int(num_clients)
        self.dtype = dtype
        self.device = device if device is not None else tree_util._default_device()
        vw = 16 // torch.empty((), dtype=dtype).element_size()
        self.row_stride = max(vw, (self.num_params + vw - 1) // vw * vw)
        from fedjax_amd import memory

        with memory.producing(self.device):  # the delta pool under memory.set_default(True)
            self.storage = torch.empty(self.num_clients, self.row_stride, dtype=dtype, device=self.device)
        if self.row_stride > self.num_params:
            self.storage[:, self.num_params:].zero_()

    # ------------------------------------------------------------------ views
    @property
    def rows(self) -> torch.Tensor:
        """[K, P] view of the deltas (row stride = ``row_stride``)."""
        return self.storage[:, : self.num_params]

    def unflatten(self, flat: torch.Tensor) -> PyTree:
        """Pytree of views into a flat P-element tensor."""
        views = [flat[o:o + n].view(s) for o, n, s in zip(self.offsets[:-1], self.sizes, self.shapes)]
        return pytree.unflatten(self.treedef, views)

    def client(self, k: int) -> PyTree:
        """Pytree of views into client k's row (write a delta through them)."""
        return self.unflatten(self.storage[k])

    def set_client(self, k: int, delta: PyTree) -> None:
        """Copy one client's delta (device or host pytree) into row k."""
        for dst, src in zip(pytree.leaves_of(self.client(k)), pytree.flatten_as(self.treedef, delta)):
            dst.copy_(tree_util._to_tensor(src), non_blocking=True)

    def fill_synthetic(self, *, seed: int = 0, amp: float = 0.01, k0: int = 0) -> "ClientDeltaSlab":
        """x[k, p] = amp * u(seed, k0 + k, p): the synthetic deltas of bench.py."""
        kernels.fill_synth(self.rows, seed=seed, amp=amp, k0=k0)
        return self

    # ------------------------------------------------------------- aggregation
    def host_weights(self, weights: Sequence) -> np.ndarray:
        """float32 weights f32(w_k) on the host."""
        if len(weights) != self.num_clients:
            raise ValueError(f"need {self.num_clients} weights, got {len(weights)}")
        return np.array([np.float32(tree_util._host_weight(x)) for x in weights], dtype=np.float32)

    def weight_vector(self, weights: Sequence) -> torch.Tensor:
        """float32 weights f32(w_k) on the device (pinned H2D, stream-ordered)."""
        return _lib.upload(torch.from_numpy(self.host_weights(weights)), self.device)

    def weighted_sum_flat(self, w_dev: torch.Tensor, *, scale=None, out: Optional[torch.Tensor] = None,
                          accumulate: bool = False, mode: str = "exact",
                          nontemporal: Optional[bool] = None, variant: int = 0,
                          reference_bf16: Optional[bool] = None) -> torch.Tensor:
        """Flat P-element fold of the slab (one launch). ``w_dev``: device weights, or host
        float32 weights (carried in the kernel arguments when the launch allows it, see
        :func:`kernels.weighted_sum_dense`). A bfloat16
        slab folds with the reference's bf16 arithmetic when ``reference_bf16`` (default:
        ``tree_util.set_bf16_semantics("reference")`` is in force and mode is exact)."""
        nbytes = self.rows.numel() * self.rows.element_size()
        nt = nbytes >= tree_util.NONTEMPORAL_MIN_BYTES if nontemporal is None else nontemporal
        if reference_bf16 is None:
            reference_bf16 = (self.dtype == torch.bfloat16 and mode == "exact"
                              and tree_util.bf16_semantics() == "reference")
        return kernels.weighted_sum_dense(
            self.rows, w_dev, scale=None if scale is None else float(np.float32(scale)), out=out,
            accumulate=accumulate, mode=mode, nontemporal=nt, variant=variant, reference_bf16=reference_bf16)

    def mean(self, weights: Sequence, *, out: Optional[torch.Tensor] = None, mode: str = "exact",
             with_norms: bool = False):
        """Weighted mean of the K rows — ``tree_mean(zip(clients, weights))`` with the
        reference's W and f32(1/W) (tree_util.py:86-96), one dense launch.

        ``with_norms=True`` also returns every client's delta l2 norm (float32[K],
        the ``delta_l2_norm`` diagnostic of examples/fed_avg.py:79-81) computed in
        the same pass over the slab: ``(mean, norms)``."""
        W = 0.0
        for x in weights:
            W += tree_util._host_weight(x)
        scale = tree_util._inverse(W)
        if with_norms and self.dtype == torch.bfloat16 and tree_util.bf16_semantics() == "reference":
            # no fused-norm kernel for the bf16 reference fold: the mean, then the norms
            if mode != "exact":
                raise ValueError("fused norms run in exact mode")
            flat = self.weighted_sum_flat(self.host_weights(weights), scale=scale, out=out)
            return self.unflatten(flat), self.l2_norms()
        if with_norms:
            if mode != "exact":
                raise ValueError("fused norms run in exact mode")
            nbytes = self.rows.numel() * self.rows.element_size()
            flat, l2sq = kernels.weighted_sum_l2_dense(
                self.rows, self.weight_vector(weights), scale=float(np.float32(scale)), out=out,
                nontemporal=nbytes >= tree_util.NONTEMPORAL_MIN_BYTES)
            return self.unflatten(flat), torch.sqrt(l2sq)
        flat = self.weighted_sum_flat(self.host_weights(weights), scale=scale, out=out, mode=mode)
        return self.unflatten(flat)

    def clipped_mean(self, weights: Sequence, max_norm: float, *,
                     out: Optional[torch.Tensor] = None) -> "tree_util.ClippedMean":
        """Weighted mean of the K rows with every client's delta clipped to l2 norm
        ``max_norm`` first: the loop of fedjax/algorithms/mime_lite.py:131-149
        (tree_clip_by_global_norm, tree_util.py:117-133, before weighting and adding) for the
        whole round, with the reference's W and f32(1/W) — clipping does not change W.

        Two passes over the slab and three small launches, no host synchronisation and no
        clipped copy: the squared norms (summed leaf by leaf, in :func:`tree_util.tree_clipped_mean`'s
        order, so that both routes form the same norms, factors and mean bit for bit over the
        same deltas), the clip factors ``c = min(1, max_norm / norm)`` on
        the device, the fold ``fl(fl(c_k x) w_k)`` with the clipped squares from the same
        pass, their combine, and the diagnostics. Returns a
        :class:`~fedjax_amd.tree_util.ClippedMean`; a float32 slab of up to 4096 clients."""
        if self.dtype != torch.float32:
            raise TypeError(f"clipped_mean needs a float32 slab, not {self.dtype}")
        if self.num_clients > tree_util._L2_MAX_CLIENTS:
            raise ValueError(f"clipped_mean supports up to {tree_util._L2_MAX_CLIENTS} clients")
        W = 0.0
        for x in weights:
            W += tree_util._host_weight(x)
        scale = tree_util._inverse(W)
        rows = self.rows
        if self.num_params == 0:  # a template of empty leaves: every norm is 0, nothing to fold
            if len(weights) != self.num_clients:
                raise ValueError(f"need {self.num_clients} weights, got {len(weights)}")
            zeros = torch.zeros(self.num_clients, dtype=torch.float32, device=self.device)
            norms, c = kernels.clip_scales(zeros, max_norm)
            clipped_norms, clipped = kernels.clip_finish(norms, c, zeros)
            flat = out if out is not None else torch.empty(0, dtype=torch.float32, device=self.device)
            return tree_util.ClippedMean(self.unflatten(flat), norms, clipped_norms, clipped)
        w_dev = self.weight_vector(weights)
        # every leaf of every row as a row of fjagg_l2sq_rows: the pytree route's reduction order
        leaf_ptrs = self.storage.data_ptr() + 4 * (np.arange(self.num_clients, dtype=np.int64)[:, None] * self.row_stride
                                                   + self.offsets[None, :-1])
        l2sq = tree_util._l2sq_table(leaf_ptrs, np.array(self.sizes, dtype=np.int64), self.device)
        norms, c = kernels.clip_scales(l2sq, max_norm)
        nbytes = rows.numel() * rows.element_size()
        flat, l2sq_clipped = kernels.clipped_sum_dense(
            rows, w_dev, c, scale=float(np.float32(scale)), out=out,
            nontemporal=nbytes >= tree_util.NONTEMPORAL_MIN_BYTES, with_clipped_l2sq=True)
        clipped_norms, clipped = kernels.clip_finish(norms, c, l2sq_clipped)
        return tree_util.ClippedMean(self.unflatten(flat), norms, clipped_norms, clipped)

    def dp_clipped_mean(self, weights: Sequence, max_norm: float, noise_stddev: float, key, *,
                        out: Optional[torch.Tensor] = None) -> "tree_util.ClippedMean":
        """:meth:`clipped_mean` with Gaussian noise of standard deviation ``noise_stddev`` added to
        the clipped mean inside the fold — both halves of DP-FedAvg in the passes and launches of
        ``clipped_mean``. Leaf ``l`` of the mean is, bit for bit,

            clipped_mean(...).mean[l] + f32(noise_stddev) * random.normal(keys[l], shape_l)

        (a float32 multiply, then a float32 add) with ``keys = random.split(key, L)`` in jax leaf
        order, the schedule of ``uniform_stochastic_quantize_pytree``; the same bits as
        :func:`tree_util.tree_dp_clipped_mean` over the same deltas. The draw happens in the fold's
        epilogue: no noise tensor, no second launch. ``norms``, ``clipped_norms`` and ``clipped``
        are ``clipped_mean``'s. The row padding past ``num_params`` is not written.

        ``key``: two uint32 words (``random.PRNGKey`` / ``split`` / ``PRNGSequence``); use each key
        once. Calibrating ``noise_stddev`` to ``max_norm`` is the caller's
        (:func:`fedjax_amd.aggregators.dp_clipped_mean_aggregator` does it for the weighted mean).

        Raises under stream capture: the key is baked into the kernel arguments, so a graph replay
        would reuse the noise, and that silently voids the privacy guarantee."""
        from fedjax_amd import random as fj_random

        kernels.refuse_capture("dp_clipped_mean")
        sd = kernels.check_noise_stddev(noise_stddev)
        key = fj_random.strict_key(key)
        if self.dtype != torch.float32:
            raise TypeError(f"dp_clipped_mean needs a float32 slab, not {self.dtype}")
        if self.num_clients > tree_util._L2_MAX_CLIENTS:
            raise ValueError(f"dp_clipped_mean supports up to {tree_util._L2_MAX_CLIENTS} clients")
        if self.num_params == 0:  # nothing to fold, nothing to draw
            return self.clipped_mean(weights, max_norm, out=out)
        L = len(self.sizes)
        if L > _lib.NOISE_MAX_LEAVES:
            raise ValueError(f"dp_clipped_mean on a slab takes up to {_lib.NOISE_MAX_LEAVES} leaves (got {L}); "
                             "use tree_util.tree_dp_clipped_mean over the client views")
        W = 0.0
        for x in weights:
            W += tree_util._host_weight(x)
        scale = tree_util._inverse(W)
        rows = self.rows
        w_dev = self.weight_vector(weights)
        noise = kernels.NoiseTable(sd, self.offsets[:-1], self.sizes, fj_random.split(key, L))
        leaf_ptrs = self.storage.data_ptr() + 4 * (np.arange(self.num_clients, dtype=np.int64)[:, None] * self.row_stride
                                                   + self.offsets[None, :-1])
        l2sq = tree_util._l2sq_table(leaf_ptrs, np.array(self.sizes, dtype=np.int64), self.device)
        norms, c = kernels.clip_scales(l2sq, max_norm)
        nbytes = rows.numel() * rows.element_size()
        flat, l2sq_clipped = kernels.dp_clipped_sum_dense(
            rows, w_dev, c, noise, scale=float(np.float32(scale)), out=out,
            nontemporal=nbytes >= tree_util.NONTEMPORAL_MIN_BYTES, with_clipped_l2sq=True)
        clipped_norms, clipped = kernels.clip_finish(norms, c, l2sq_clipped)
        return tree_util.ClippedMean(self.unflatten(flat), norms, clipped_norms, clipped)

    def grouped_mean(self, weights: Sequence, group_ids: Sequence[int], num_groups: int, *,
                     out: Optional[torch.Tensor] = None) -> list:
        """Per-group weighted means of the rows in ONE pass over the slab: the expectation step
        of fedjax/algorithms/hyp_cluster.py:268-303. Client k belongs to group ``group_ids[k]``
        in ``[0, num_groups)``, or to none with -1 (a dropped or unsampled client: its row is
        never loaded, so its inf or NaN touch nothing). For each group, in client order,

            W_g = sum of its members' weights; s = +0; s = s + x_m * w_m; mean_g = s * f32(1/W_g)

        the reference's running sum onto ``tree_zeros_like`` (so a sum of -0 products is +0).
        Returns a list of ``num_groups`` pytrees of the template's structure — views into one
        ``[G, row_stride]`` result (``out`` if given) — with ``None`` for every group whose total
        weight is not > 0 (no members, a zero, negative or NaN total; hyp_cluster.py:298-302);
        such a group's row of the result is not written. A float32 slab; no host synchronisation.

        The member tables travel as one pinned upload, which a graph capture cannot record
        safely; the tables of the latest call stay on the device, so a capture of the SAME
        weights and ids (after one eager call) launches without an upload and replays with
        rewritten deltas; any other capture is refused. A later call on another stream waits
        for the upload through an event; a capture cannot wait on an event recorded outside
        it, so the upload must be complete when the capture begins (``torch.cuda.graph``
        synchronises the device on entry; with ``CUDAGraph.capture_begin`` synchronise first)."""
        if self.dtype != torch.float32:
            raise TypeError(f"grouped_mean needs a float32 slab, not {self.dtype}")
        K, G = self.num_clients, int(num_groups)
        ids = kernels.check_group_ids(group_ids, K, G)
        w = self.host_weights(weights)
        totals = [0] * G  # W_g summed as hyp_cluster.py:282,292 does, from the int 0
        for k in np.flatnonzero(ids >= 0):
            totals[ids[k]] += tree_util._host_weight(weights[k])
        alive = np.array([bool(W > 0) for W in totals])
        ids = np.where((ids >= 0) & alive[np.maximum(ids, 0)], ids, -1)  # a group without a mean is not folded
        scales = np.array([np.float32(tree_util._inverse(W)) if a else 0 for W, a in zip(totals, alive)], np.float32)
        key = (w.tobytes(), ids.tobytes(), scales.tobytes())
        cached = getattr(self, "_group_tables", None)
        capturing = torch.cuda.is_current_stream_capturing()
        stream = torch.cuda.current_stream(self.device)
        if cached is not None and cached[0] == key:
            tables, up_stream, uploaded = cached[1:]
            if capturing:  # the graph reads this buffer on every replay: it lives as long as the slab
                self._captured_tables = getattr(self, "_captured_tables", []) + [tables]
            elif stream != up_stream:  # uploaded on another stream: this one waits for the copy
                stream.wait_event(uploaded)
        else:
            tables = kernels.GroupTables(w, ids, G, scales).upload(self.device)  # (refused under capture)
            uploaded = torch.cuda.Event()
            uploaded.record(stream)
            self._group_tables = (key, tables, stream, uploaded)
        if out is None:
            out = torch.empty(G, self.row_stride, dtype=torch.float32, device=self.device)
        if tuple(out.shape) != (G, self.row_stride) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 [{G}, {self.row_stride}] tensor")
        rows = self.rows
        nbytes = tables.M * self.num_params * 4
        if self.num_params:  # (a template of empty leaves: the means are empty too, nothing to fold)
            kernels.grouped_sum_dense(rows, w, ids, G, out=out[:, : self.num_params], tables=tables,
                                      nontemporal=nbytes >= tree_util.NONTEMPORAL_MIN_BYTES)
        return [self.unflatten(out[g]) if alive[g] else None for g in range(G)]

    def trimmed_mean(self, trim, *, bucket_size: Optional[int] = None, perm=None,
                     out: Optional[torch.Tensor] = None) -> PyTree:
        """Coordinate-wise trimmed mean of the K rows (Yin et al., ICML 2018): in every coordinate
        the ``t`` smallest and the ``t`` largest client values are dropped and the rest averaged,
        so up to ``t`` clients that upload ``inf``, ``NaN`` or huge values in a coordinate do not
        reach the result. ``trim`` is the int count ``t``, or a float fraction ``0 <= beta < 0.5``
        giving ``t = floor(beta * K)``; a bool is refused. One launch that reads every delta
        once, nothing uploaded (graph-capturable), no K x P temporary.

        Values are ranked by the total order ``-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN``
        (ties by client index); the kept values are added in client order like
        :meth:`mean` adds and multiplied by f32(1 / (K - 2t)), so ``trim=0`` is bit for bit
        ``mean([1] * K)``. There are no weights: a robust aggregate that let a client scale its
        own vote would not be robust. A float32 slab of up to 128 clients. Returns the
        template's pytree (views into ``out`` if given: float32, ``num_params`` elements).

        ``bucket_size=s`` is bucketing (Karimireddy, He and Jaggi, ICLR 2022): the
        clients are averaged in ``B = ceil(K / s)`` buckets of ``s`` and the rule runs over the
        bucket means, which helps on heterogeneous clients and lifts the limit to 4096 clients
        (``B <= 128``). Bucket ``j`` holds the clients ``perm[j*s + i]``; its mean is the first
        member verbatim, the others added in table order, times f32(1 / n_j) — a short last
        bucket is divided by its own size. ``trim`` then counts BUCKETS (a fraction gives
        ``floor(beta * B)``), ties go by bucket index and the scale is f32(1 / (B - 2t)); ``f``
        bad clients can spoil ``f`` buckets out of ``B``, so the tolerable fraction of bad
        clients shrinks by ``s``. ``perm`` is ``None`` (consecutive clients, unshuffled), a host
        int sequence (checked to be a permutation of ``range(K)`` and uploaded, which a stream
        capture refuses), or an int32 device tensor of ``K`` entries such as
        :func:`fedjax_amd.random.permutation` returns (used as it is, never read by the host:
        nothing is uploaded, the call can be captured and each replay reads the table afresh;
        the kernel clamps its entries into ``[0, K)``). Still one launch and no temporary; the
        bucket means are formed inside the column kernel, which reads every delta twice.
        ``bucket_size=1`` without ``perm`` is bit for bit the unbucketed result. ``perm`` without
        ``bucket_size`` is a ``ValueError``."""
        if self.dtype != torch.float32:
            raise TypeError(f"trimmed_mean needs a float32 slab, not {self.dtype}")
        K = self.num_clients
        if bucket_size is None:
            if perm is not None:
                raise ValueError("perm orders the clients of a bucketed aggregate: pass bucket_size too")
            t = kernels.trim_count(trim, K)
        else:
            B = kernels.bucket_count(K, bucket_size)
            t = kernels.bucket_trim_count(trim, B)
            perm = kernels.check_bucket_perm(perm, K)
        if self.num_params == 0:  # a template of empty leaves: nothing to launch
            flat = out if out is not None else torch.empty(0, dtype=torch.float32, device=self.device)
            return self.unflatten(flat)
        rows = self.rows
        nbytes = rows.numel() * rows.element_size()
        if bucket_size is None:
            flat = kernels.trim_dense(rows, t, scale=float(np.float32(tree_util._inverse(K - 2 * t))), out=out,
                                      nontemporal=nbytes >= tree_util.NONTEMPORAL_MIN_BYTES)
        else:
            flat = kernels.trim_bucket_dense(rows, int(bucket_size), t, perm=kernels.bucket_perm_device(perm, self.device),
                                             scale=float(np.float32(tree_util._inverse(B - 2 * t))), out=out,
                                             nontemporal=nbytes >= tree_util.NONTEMPORAL_MIN_BYTES)
        return self.unflatten(flat)

    def median(self, *, bucket_size: Optional[int] = None, perm=None, out: Optional[torch.Tensor] = None) -> PyTree:
        """Coordinate-wise median of the K rows: :meth:`trimmed_mean` at ``t = (K-1) // 2``. Odd
        K gives the middle value verbatim, even K ``fl(fl(a + b) * 0.5)`` of the two middle
        values (a before b in client order); ``np.median``'s bits on finite data. Weights play
        no part. A float32 slab of up to 128 clients. With ``bucket_size`` (and ``perm``) as
        :meth:`trimmed_mean` takes them: the median of the ``B`` bucket means, ``t = (B-1) // 2``,
        for up to 4096 clients."""
        if self.dtype != torch.float32:
            raise TypeError(f"median needs a float32 slab, not {self.dtype}")
        if bucket_size is None:
            if perm is not None:
                raise ValueError("perm orders the clients of a bucketed aggregate: pass bucket_size too")
            kernels.trim_count(0, self.num_clients)
            return self.trimmed_mean((self.num_clients - 1) // 2, out=out)
        B = kernels.bucket_count(self.num_clients, bucket_size)
        return self.trimmed_mean((B - 1) // 2, bucket_size=bucket_size, perm=perm, out=out)

    def mean_around_median(self, keep, *, rows: Optional[Sequence[int]] = None,
                           out: Optional[torch.Tensor] = None) -> PyTree:
        """The mean around the median of the rows ("MeaMed", Xie et al. 2018; the coordinate-wise
        stage of Bulyan): in every coordinate, the mean of the ``keep`` client values closest to
        the coordinate's lower median ``s_mid``, ``mid = (K-1) // 2``. ``keep`` is an int in
        ``[1, K]``; a bool is refused. ``rows``: the participating clients, strictly ascending
        row indices, at most 128 of a slab of up to 1024 rows (default: all rows of a slab of up
        to 128); ``K`` is then their number and no other row is read. One launch, nothing
        uploaded (the row table travels in the kernel arguments: graph-capturable), no
        temporary.

        The order, the ties and the sum are :meth:`trimmed_mean`'s; a value's distance from the
        median is ``|fl(v - med)|`` in float32 (0 for the median's own bits, ``+inf`` where the
        difference is NaN) and the kept sorted positions are a window around ``mid`` grown
        towards the strictly closer side, the lower side on a tie. The result is multiplied by
        f32(1 / keep): ``keep = K`` is bit for bit ``mean([1] * K)``, ``keep = 1`` the lower
        median verbatim. There are no weights. A float32 slab. Returns the template's pytree
        (views into ``out`` if given: float32, ``num_params`` elements)."""
        if self.dtype != torch.float32:
            raise TypeError(f"mean_around_median needs a float32 slab, not {self.dtype}")
        if rows is not None:
            if self.num_clients > kernels.MEAMED_MAX_SLAB_ROWS:
                raise ValueError(f"a row table selects from a slab of up to {kernels.MEAMED_MAX_SLAB_ROWS} "
                                 f"clients, got K = {self.num_clients}")
            rows = kernels._row_table(rows, self.num_clients)
        M = self.num_clients if rows is None else int(rows.size)
        keep = kernels.keep_count(keep, M)
        if self.num_params == 0:  # a template of empty leaves: nothing to launch
            flat = out if out is not None else torch.empty(0, dtype=torch.float32, device=self.device)
            return self.unflatten(flat)
        flat = kernels.meamed_dense(self.rows, keep, rows, scale=float(np.float32(tree_util._inverse(keep))), out=out,
                                    nontemporal=M * self.num_params * 4 >= tree_util.NONTEMPORAL_MIN_BYTES)
        return self.unflatten(flat)

    def bulyan(self, num_byzantine, *, select: str = "host"):
        """Bulyan (El Mhamdi, Guerraoui and Rouault, ICML 2018) over the rows: Krum iterated
        ``theta = K - 2f`` times on the shrinking set of clients not yet chosen
        (:func:`fedjax_amd.robust.bulyan_select`, ``f = num_byzantine``), then
        :meth:`mean_around_median` with ``keep = theta - 2f`` over the chosen rows in ascending
        order. ``K >= 4f + 3``.

        :meth:`gram`, ONE device-to-host copy of the K x K float64 Gram, the selection on the
        host, then one launch whose row table names the chosen clients — the others are never
        loaded, so up to ``f`` clients full of NaN, inf or 1e30 cannot reach the result, and a
        client that hides one huge coordinate behind a small distance is cut by the
        coordinate-wise stage. There are no client weights. Returns a
        :class:`~fedjax_amd.tree_util.BulyanResult`; ``mean`` is ``None`` when fewer than
        ``2f + 1`` clients could be selected. A float32 slab of up to 1024 clients with
        ``K - 2f <= 128``. Raises under stream capture.

        ``select="device"`` keeps the round on the device: :meth:`gram`, ``fjagg_bulyan_select``
        (the same selection, bit for bit), then the second stage reading its row table, count,
        keep count and scale from device memory (``fjagg_meamed_dense_dev``: the same column
        routine, so the same bits as the host route's mean). No device-to-host copy, no
        synchronisation, nothing uploaded: the round can be captured into a graph and replayed
        over rewritten deltas, and each replay selects afresh. The argument checks and their
        exceptions are the same. Returns a :class:`~fedjax_amd.tree_util.DeviceBulyanResult` of
        device tensors; ``mean`` is all +0 when fewer than ``2f + 1`` clients could be selected
        (never ``None``)."""
        if kernels.check_select(select):
            if self.dtype != torch.float32:
                raise TypeError(f"bulyan needs a float32 slab, not {self.dtype}")
            f = tree_util._check_bulyan_args(self.num_clients, num_byzantine)
            gram = self.gram()
            selected, count, step_scores, tables = kernels.bulyan_select_device(gram, f)
            out = torch.empty(self.row_stride, dtype=torch.float32, device=self.device)
            if self.num_params:
                nbytes = tables.M_max * self.num_params * 4
                kernels.meamed_dense_device(self.rows, tables, out=out[: self.num_params],
                                            nontemporal=nbytes >= tree_util.NONTEMPORAL_MIN_BYTES)
            # (a template of empty leaves: nothing to launch; the padding past num_params is never shown)
            return tree_util.DeviceBulyanResult(self.unflatten(out), selected, count, tables.keep, step_scores, gram)
        kernels.refuse_capture("bulyan", kernels._TWO_PASS)
        if self.dtype != torch.float32:
            raise TypeError(f"bulyan needs a float32 slab, not {self.dtype}")
        f = tree_util._check_bulyan_args(self.num_clients, num_byzantine)
        gram = self.gram()
        selected, members, keep = tree_util._bulyan_plan(gram.cpu().numpy(), f)
        mean = self.mean_around_median(keep, rows=members) if keep else None
        return tree_util.BulyanResult(mean, selected, keep, gram)

    def gram(self, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Gram matrix ``G[i][j] = <row i, row j>`` of the K deltas as a float64 ``[K, K]`` device
        tensor: one pass over the slab on the f32 matrix instruction
        (:func:`kernels.gram_dense`), no host synchronisation, nothing uploaded. What Krum and
        the geometric median are functions of (:mod:`fedjax_amd.robust`). Bitwise reproducible
        and symmetric; a client holding a NaN or inf makes only its own row and column
        non-finite. A float32 slab of up to 1024 clients."""
        if self.dtype != torch.float32:
            raise TypeError(f"gram needs a float32 slab, not {self.dtype}")
        K = kernels._check_gram_clients(self.num_clients)
        if self.num_params == 0:  # a template of empty leaves: every inner product is the empty sum
            if out is None:
                return torch.zeros(K, K, dtype=torch.float64, device=self.device)
            return kernels._check_gram_out(out, K, self.device).zero_()
        return kernels.gram_dense(self.rows, out=out)

    def _fold_selected(self, tables: "kernels.DeviceGroupTables") -> PyTree:
        """The device routes' second pass: a zeroed result (a fill kernel, so a graph replay zeroes
        too), then the grouped fold over the member tables a select kernel wrote
        (:func:`kernels.grouped_sum_dense_device`), which writes nothing for an empty group."""
        out = torch.empty(self.row_stride, dtype=torch.float32, device=self.device)
        out.zero_()
        if self.num_params:  # (a template of empty leaves: nothing to fold)
            nbytes = tables.M_max * self.num_params * 4
            kernels.grouped_sum_dense_device(self.rows, tables, out[: self.num_params],
                                             nontemporal=nbytes >= tree_util.NONTEMPORAL_MIN_BYTES)
        return self.unflatten(out)

    def krum(self, num_byzantine, num_selected=1, *, select: str = "host", bucket_size: Optional[int] = None,
             perm=None):
        """Krum (``num_selected = 1``) and multi-Krum (Blanchard et al., NeurIPS 2017) over the
        rows: client i's score is the sum of its ``K - f - 2`` smallest squared distances to the
        other clients, ``f = num_byzantine``, and the ``num_selected`` clients of smallest
        score are averaged (ties to the lower index). ``K >= 2f + 3``, ``1 <= num_selected <= K - f``.

        :meth:`gram`, ONE device-to-host copy of the K x K float64 Gram, the selection on the
        host, then ``grouped_mean([1] * K, ids, 1)[0]`` with id 0 for the selected clients and
        -1 for the rest — which are never loaded, so up to ``f`` clients full of NaN, inf or
        1e30 cannot reach the result. ``num_selected = 1`` gives the chosen client's delta
        (times f32(1), from a +0 start). There are no client weights. Returns a
        :class:`~fedjax_amd.tree_util.KrumResult`; ``mean`` is ``None`` when no client has a
        finite score. A float32 slab of up to 1024 clients. Raises under stream capture.

        ``select="device"`` keeps the round on the device: :meth:`gram`, ``fjagg_krum_select``
        (the same scores and winners, bit for bit), the result zeroed, then the grouped fold over
        the member tables the kernel wrote. No device-to-host copy, no synchronisation, nothing
        uploaded: the round can be captured into a graph and replayed over rewritten deltas, and
        each replay selects afresh. The argument checks and their exceptions are the same.
        Returns a :class:`~fedjax_amd.tree_util.DeviceKrumResult` of device tensors; ``mean`` is
        all +0 when no client has a finite score (never ``None``).

        ``bucket_size=s`` is bucketing (Karimireddy, He and Jaggi, ICLR 2022): Krum
        over the means of ``B = ceil(K / s)`` buckets of the rows ``perm[j*s + i]`` (``perm``: a
        host int sequence, a permutation of ``range(K)``, or ``None`` for consecutive rows). No
        third pass: the bucket means' Gram is :func:`fedjax_amd.robust.bucket_gram` of
        :meth:`gram`, the argument checks run on ``B`` and ``f`` counts buckets. The mean is
        ``grouped_mean(w, ids, 1)[0]`` with id 0 for the members of the selected buckets, -1 for
        everyone else, and integer weights that make it the mean of the selected bucket means
        (all 1 unless the short last bucket is selected beside full ones). Returns a
        :class:`~fedjax_amd.tree_util.BucketedKrumResult`: ``selected`` and ``scores`` are per
        bucket, ``members`` names the clients. Host selection only: ``select="device"`` with
        ``bucket_size`` is a ``ValueError`` before any pass over the deltas."""
        if bucket_size is None and perm is not None:
            raise ValueError("perm orders the clients of a bucketed aggregate: pass bucket_size too")
        if bucket_size is not None:
            from fedjax_amd import robust

            kernels.check_select(select)
            if select != "host":
                raise ValueError('the bucketed selection is host-only: bucket_size needs select="host"')
            kernels.refuse_capture("krum", kernels._TWO_PASS)
            if self.dtype != torch.float32:
                raise TypeError(f"krum needs a float32 slab, not {self.dtype}")
            B, perm = tree_util._bucket_args(self.num_clients, bucket_size, perm)
            robust.check_krum_args(B, num_byzantine, num_selected)
            gram = self.gram()
            selected, scores, w, ids, members = tree_util._bucket_krum_plan(gram.cpu().numpy(), bucket_size, perm,
                                                                            num_byzantine, num_selected)
            mean = self.grouped_mean(w, ids, 1)[0] if len(selected) else None
            return tree_util.BucketedKrumResult(mean, selected, scores, gram, members)
        if kernels.check_select(select):
            if self.dtype != torch.float32:
                raise TypeError(f"krum needs a float32 slab, not {self.dtype}")
            tree_util._check_krum_args_only(self.num_clients, num_byzantine, num_selected)
            gram = self.gram()
            scores, selected, count, tables = kernels.krum_select_device(gram, num_byzantine, num_selected)
            return tree_util.DeviceKrumResult(self._fold_selected(tables), selected, count, scores, gram)
        kernels.refuse_capture("krum", kernels._TWO_PASS)
        if self.dtype != torch.float32:
            raise TypeError(f"krum needs a float32 slab, not {self.dtype}")
        tree_util._check_krum_args(self.num_clients, num_byzantine, num_selected)
        gram = self.gram()
        selected, scores, w, ids = tree_util._krum_plan(gram.cpu().numpy(), num_byzantine, num_selected)
        mean = self.grouped_mean(w, ids, 1)[0] if len(selected) else None
        return tree_util.KrumResult(mean, selected, scores, gram)

    def geometric_median(self, weights: Optional[Sequence] = None, *, iterations=4,
                         nu=1e-6, select: str = "host", bucket_size: Optional[int] = None, perm=None):
        """The geometric median of the rows by the smoothed Weiszfeld algorithm ("RFA", Pillutla
        et al., IEEE TSP 2022), ``weights`` the clients' positive weights alpha (default all 1).
        All ``iterations`` run on the host over the Gram matrix
        (:func:`fedjax_amd.robust.weiszfeld_weights`), so the slab is read twice whatever
        ``iterations`` is: :meth:`gram`, ONE device-to-host copy, then
        ``grouped_mean(float32(a), ids, 1)[0]`` with id -1 (never loaded, weight 0) for a client
        with a non-finite value. ``iterations = 0`` is the alpha-weighted mean of the usable
        clients. Returns a :class:`~fedjax_amd.tree_util.GeometricMedianResult`; ``median`` is
        ``None`` when no client is usable. A float32 slab of up to 1024 clients. Raises under
        stream capture.

        ``select="device"`` keeps the round on the device: :meth:`gram`,
        ``fjagg_weiszfeld_select`` (the same rule with the order of every sum pinned, so the
        weights agree with the host route's to a few float64 roundings, not bit for bit), the
        result zeroed, then the grouped fold over the tables the kernel wrote. No device-to-host
        copy and no synchronisation; ``weights`` are uploaded once (which a capture refuses),
        ``None`` uploads nothing and can be captured. The argument checks and their exceptions
        are the same. Returns a :class:`~fedjax_amd.tree_util.DeviceGeometricMedianResult`;
        ``median`` is all +0 when no client is usable (never ``None``).

        ``bucket_size=s`` is bucketing (as :meth:`krum` takes it, with ``perm``): the geometric
        median of the ``B`` bucket means. ``weiszfeld_weights`` over the bucket Gram gives ``a_b``
        and every member of bucket ``b`` folds with ``f32(a_b / n_b)``; in the result ``weights``
        are those per-CLIENT fold weights and ``distances`` are per BUCKET. Client ``weights``
        together with ``bucket_size``, and ``select="device"`` with ``bucket_size``, are
        ``ValueError`` before any pass over the deltas."""
        if bucket_size is None and perm is not None:
            raise ValueError("perm orders the clients of a bucketed aggregate: pass bucket_size too")
        if bucket_size is not None:
            kernels.check_select(select)
            if select != "host":
                raise ValueError('the bucketed selection is host-only: bucket_size needs select="host"')
            if weights is not None:
                raise ValueError("client weights and bucket_size cannot be combined: a bucket mean has no client "
                                 "weights")
            kernels.refuse_capture("geometric_median", kernels._TWO_PASS)
            if self.dtype != torch.float32:
                raise TypeError(f"geometric_median needs a float32 slab, not {self.dtype}")
            _, perm = tree_util._bucket_args(self.num_clients, bucket_size, perm)
            tree_util._check_median_iterations(iterations, nu)
            gram = self.gram()
            w32, d, ids = tree_util._bucket_median_plan(gram.cpu().numpy(), bucket_size, perm, iterations, nu)
            median = self.grouped_mean(w32, ids, 1)[0] if (ids >= 0).any() else None
            return tree_util.GeometricMedianResult(median, w32, d, gram)
        if kernels.check_select(select):
            if self.dtype != torch.float32:
                raise TypeError(f"geometric_median needs a float32 slab, not {self.dtype}")
            weights = None if weights is None else list(weights)
            tree_util._check_median_args(self.num_clients, weights, iterations, nu)
            tree_util._check_median_iterations(iterations, nu)
            alpha = None if weights is None else np.array([tree_util._host_weight(w) for w in weights], np.float64)
            gram = self.gram()
            _, d, a32, count, tables = kernels.weiszfeld_select_device(gram, alpha, nu, iterations)
            return tree_util.DeviceGeometricMedianResult(self._fold_selected(tables), a32, d, count, gram)
        kernels.refuse_capture("geometric_median", kernels._TWO_PASS)
        if self.dtype != torch.float32:
            raise TypeError(f"geometric_median needs a float32 slab, not {self.dtype}")
        weights = None if weights is None else list(weights)
        tree_util._check_median_args(self.num_clients, weights, iterations, nu)
        gram = self.gram()
        a32, d, ids = tree_util._median_plan(gram.cpu().numpy(), weights, iterations, nu)
        median = self.grouped_mean(a32, ids, 1)[0] if (ids >= 0).any() else None
        return tree_util.GeometricMedianResult(median, a32, d, gram)

    def _flat_center(self, center, name: str = "center") -> torch.Tensor:
        """``center`` of :meth:`centered_clip` as a flat float32 [num_params] device tensor: zeros for
        ``None``, the tensor itself when it is flat, a fresh row filled from a pytree's leaves."""
        P = self.num_params
        if center is None:
            return torch.zeros(P, dtype=torch.float32, device=self.device)
        if isinstance(center, torch.Tensor):
            if center.dtype != torch.float32:
                raise TypeError(f"{name} must be float32, not {center.dtype}")
            if center.dim() != 1 or center.numel() != P or not center.is_contiguous() or center.device != self.storage.device:
                raise ValueError(f"a flat {name} is a contiguous float32 [{P}] tensor on {self.storage.device}")
            return center
        leaves = pytree.flatten_as(self.treedef, center)
        flat = torch.empty(P, dtype=torch.float32, device=self.device)
        for l, (dst, src, shape) in enumerate(zip(pytree.leaves_of(self.unflatten(flat)), leaves, self.shapes)):
            if not isinstance(src, torch.Tensor) or src.dtype != torch.float32:
                raise TypeError(f"{name} leaf {l} must be a float32 tensor")
            if tuple(src.shape) != shape or src.device != self.storage.device:
                raise ValueError(f"{name} leaf {l} must have shape {shape} on {self.storage.device}")
            dst.copy_(src)
        return flat

    def _center_leaf_table(self) -> torch.Tensor:
        """The slab's leaf-row table ``off[L] | n[L]`` on the device: constant for the slab's life,
        so it is uploaded on first use (refused under capture, :func:`_lib.upload`) and kept. A call
        on another stream waits for the upload through an event; a capture cannot wait on an event
        recorded outside it, so the upload must be complete when a capture begins
        (``torch.cuda.graph`` synchronises the device on entry)."""
        stream = torch.cuda.current_stream(self.device)
        cached = getattr(self, "_center_tab", None)
        if cached is None:
            host = np.concatenate([self.offsets[:-1], np.array(self.sizes, dtype=np.int64)]).astype(np.int64)
            tab = _lib.upload(torch.from_numpy(host), self.device)
            uploaded = torch.cuda.Event()
            uploaded.record(stream)
            cached = self._center_tab = (tab, stream, uploaded)
        elif stream != cached[1] and not torch.cuda.is_current_stream_capturing():
            stream.wait_event(cached[2])
        return cached[0]

    def centered_clip(self, tau, center=None, *, iterations: int = 1,
                      out: Optional[torch.Tensor] = None) -> "tree_util.CenteredClip":
        """Centered clipping of the K rows (Karimireddy, He and Jaggi, ICML 2021): the mean of the
        rows, each clipped to l2 distance ``tau`` from the centre, taken around that centre,
        ``iterations`` times from ``center`` — the previous round's aggregate: a flat float32
        ``[num_params]`` tensor, a pytree of the template's structure, or ``None`` for zeros.
        The arithmetic is :func:`fedjax_amd.tree_util.tree_centered_clip`'s, and the result is bit
        for bit that function's over the same deltas (the distances add up leaf by leaf in both).
        There are no weights.

        ``out``: a flat float32 ``[num_params]`` tensor for the new centre; ``out is center`` is
        allowed (every iteration after the first runs in place anyway), a partial overlap is not, and
        neither is an ``out`` inside the slab's own rows (they are read while ``out`` is written).
        Two passes over the slab and two small launches per iteration, no host synchronisation.
        The only upload is the slab's leaf table, once, on the first call: every later call,
        one under stream capture included, uploads nothing — after one eager call a round with
        ``out=center`` can be captured and replayed with rewritten deltas. A first call under
        capture raises. Returns a :class:`~fedjax_amd.tree_util.CenteredClip` whose ``center`` is
        the template's pytree of views into ``out``; a float32 slab of up to 4096 clients."""
        if self.dtype != torch.float32:
            raise TypeError(f"centered_clip needs a float32 slab, not {self.dtype}")
        K, P = self.num_clients, self.num_params
        tau, iterations = kernels.check_center_args(K, tau, iterations)
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32):
            raise TypeError("out must be a float32 tensor")
        if out is not None and (out.dim() != 1 or out.numel() != P or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of {P} elements")
        if P == 0:  # a template of empty leaves: every distance is 0, nothing to launch
            flat = out if out is not None else torch.empty(0, dtype=torch.float32, device=self.device)
            return tree_util.CenteredClip(self.unflatten(flat),
                                          torch.zeros(iterations, K, dtype=torch.float32, device=self.device),
                                          torch.ones(iterations, K, dtype=torch.float32, device=self.device))
        tab = self._center_leaf_table()
        rows = self.rows
        flat, distances, factors = kernels.centered_clip_dense(
            rows, tau, self._flat_center(center), iterations=iterations, out=out, leaf_table=tab,
            max_n=max(self.sizes), nontemporal=rows.numel() * 4 >= tree_util.NONTEMPORAL_MIN_BYTES)
        return tree_util.CenteredClip(self.unflatten(flat), distances, factors)

    def fltrust(self, server_delta, *, out: Optional[torch.Tensor] = None) -> "tree_util.FLTrustResult":
        """FLTrust over the K rows (Cao, Fang, Liu and Gong, NDSS 2021): every client is weighed by
        the ReLU of the cosine between its delta and ``server_delta`` — the delta the server computed
        itself on a small trusted dataset — rescaled to that delta's norm, and the trust-weighted
        mean is taken. ``server_delta`` is a flat float32 ``[num_params]`` tensor or a pytree of the
        template's structure (copied into a flat row on the device). The arithmetic is
        :func:`fedjax_amd.tree_util.tree_fltrust`'s, and every field of the result is bit for bit
        that function's over the same deltas (the sums add up leaf by leaf in both). There are no
        weights.

        ``out``: a flat float32 ``[num_params]`` tensor for the mean; it must overlap neither the
        slab nor ``server_delta``. Two reads of the slab — the second skips every client that was
        gated out — and a handful of small launches, no host synchronisation. The only upload is
        the slab's leaf table, once, on the first call of this or of :meth:`centered_clip`: every
        later call, one under stream capture included, uploads nothing — after one eager call a
        round can be captured and replayed over rewritten deltas and a rewritten server delta, and
        each replay selects afresh. A first call under capture raises. Returns a
        :class:`~fedjax_amd.tree_util.FLTrustResult` of device tensors whose ``mean`` is the
        template's pytree of views into ``out``, all +0 when nobody is trusted; a float32 slab of
        up to 4096 clients."""
        if self.dtype != torch.float32:
            raise TypeError(f"fltrust needs a float32 slab, not {self.dtype}")
        K, P = kernels.check_fltrust_clients(self.num_clients), self.num_params
        if server_delta is None:
            raise ValueError("fltrust needs a server_delta (there is no default: the rule has no other anchor)")
        if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32):
            raise TypeError("out must be a float32 tensor")
        if out is not None and (out.dim() != 1 or out.numel() != P or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous float32 tensor of {P} elements")
        if len(self.sizes) > 65535:
            raise ValueError(f"fltrust takes up to 65535 leaves, got {len(self.sizes)}")
        server = self._flat_center(server_delta, "server_delta")
        if P == 0:  # a template of empty leaves: every sum is the empty sum, nobody is trusted
            flat = out if out is not None else torch.empty(0, dtype=torch.float32, device=self.device)
            return tree_util.FLTrustResult(self.unflatten(flat), *tree_util._fltrust_nobody(K, self.device))
        tab = self._center_leaf_table()
        rows = self.rows
        flat, d = kernels.fltrust_dense(rows, server, out=out, leaf_table=tab, max_n=max(self.sizes),
                                        nontemporal=rows.numel() * 4 >= tree_util.NONTEMPORAL_MIN_BYTES)
        return tree_util.FLTrustResult(self.unflatten(flat), d.trust, d.cosines, d.factors, d.norms, d.server_norm,
                                       d.count, d.total)

    def _topk_weight_vector(self, weights: Sequence) -> torch.Tensor:
        """The float32 weights on the device for :meth:`topk_mean`. The vector of the latest call
        stays on the device, so a capture with the SAME weights (after one eager call) launches
        without an upload; any other capture is refused by the pinned upload, as in
        :meth:`grouped_mean` (whose notes on streams and capture apply)."""
        w = self.host_weights(weights)
        key = w.tobytes()
        cached = getattr(self, "_topk_weights", None)
        stream = torch.cuda.current_stream(self.device)
        if cached is not None and cached[0] == key:
            w_dev, up_stream, uploaded = cached[1:]
            if torch.cuda.is_current_stream_capturing():  # the graph reads this buffer on every replay
                self._captured_tables = getattr(self, "_captured_tables", []) + [w_dev]
            elif stream != up_stream:
                stream.wait_event(uploaded)
            return w_dev
        w_dev = _lib.upload(torch.from_numpy(w), self.device)  # (refused under capture)
        uploaded = torch.cuda.Event()
        uploaded.record(stream)
        self._topk_weights = (key, w_dev, stream, uploaded)
        return w_dev

    def _topk_keep(self, what: str, k) -> int:
        if self.dtype != torch.float32:
            raise TypeError(f"{what} needs a float32 slab, not {self.dtype}")
        kernels.check_topk_clients(self.num_clients)
        if self.num_params == 0:  # a template of empty leaves: nothing to select from
            if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, float, np.integer, np.floating)):
                raise TypeError("k must be an int count or a float fraction in (0, 1], not "
                                f"{type(k).__name__}")
            return 0
        return kernels.topk_count(k, self.num_params)

    def topk_thresholds(self, k):
        """``(thresholds, sent)`` of :meth:`topk_mean` alone: per client the magnitude threshold of
        its ``k`` largest coordinates (float32 [K]) and the number of coordinates it would transmit
        (int32 [K]). Three passes over the slab, nothing uploaded, no host synchronisation:
        graph-capturable."""
        c = self._topk_keep("topk_thresholds", k)
        return kernels.topk_select_dense(self.rows, c)

    def topk_mean(self, weights: Sequence, k, *, out: Optional[torch.Tensor] = None) -> "tree_util.TopKMean":
        """Weighted mean of the K rows with every client's delta sparsified to its ``k``
        largest-magnitude coordinates first (top-k sparsification, the most widely used
        compression rule of federated learning). ``k`` is an int count ``1 <= k <= num_params`` or
        a float fraction ``0 < beta <= 1`` giving ``max(1, floor(beta * num_params))``; a bool is
        refused. The selection is over the client's whole row (all leaves together).

        The magnitude of ``v`` is the integer ``bits(v) & 0x7fffffff``, so ``|NaN| > inf > ... >
        subnormals > 0``; ``T_k`` is the exact ``k``-th largest magnitude of row ``k`` and a
        coordinate is kept iff its magnitude is ``>= T_k``: all ties at the threshold are kept (at
        least ``k`` coordinates survive), and a NaN is kept first — this is compression, not
        robustness. A dropped coordinate counts as ``+0`` in :meth:`mean`'s fold (a kept ``-0``
        passes verbatim), with the same ``W`` and ``f32(1/W)``: the result is bit for bit
        ``mean(weights)`` of a slab holding the sparsified rows, and ``k = num_params`` is bit for
        bit ``mean(weights)``.

        Three histogram passes and one fold over the slab and four small launches; no sort, no
        sparsified copy, no host synchronisation. The only upload is the weight vector, kept on
        the device: after one eager call a round with the same weights can be captured into a
        graph and replayed over rewritten deltas, and every replay selects afresh. Returns a
        :class:`~fedjax_amd.tree_util.TopKMean` of the template's pytree (views into ``out`` if
        given: float32, ``num_params`` elements) and the device diagnostics ``thresholds`` and
        ``sent``. A float32 slab of up to 4096 clients, fewer than 2^31 parameters."""
        c = self._topk_keep("topk_mean", k)
        W = 0.0
        for x in weights:
            W += tree_util._host_weight(x)
        scale = tree_util._inverse(W)
        if self.num_params == 0:
            if len(weights) != self.num_clients:
                raise ValueError(f"need {self.num_clients} weights, got {len(weights)}")
            flat = out if out is not None else torch.empty(0, dtype=torch.float32, device=self.device)
            thr = torch.zeros(self.num_clients, dtype=torch.float32, device=self.device)
            return tree_util.TopKMean(self.unflatten(flat), thr, torch.zeros_like(thr, dtype=torch.int32))
        w_dev = self._topk_weight_vector(weights)
        flat, thr, sent = kernels.topk_mean_dense(self.rows, w_dev, c, scale=scale, out=out)
        return tree_util.TopKMean(self.unflatten(flat), thr, sent)

    def l2_norms(self) -> torch.Tensor:
        """Per-client delta l2 norms (float32[K]) in one pass over the slab."""
        return torch.sqrt(kernels.l2_squared_dense(self.rows))


__all__ = ["ClientDeltaSlab"]
