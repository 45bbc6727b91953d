"""Aggregator interface and the weighted-mean aggregator.

Mirror of google/fedjax 0.0.17 ``fedjax/aggregators/aggregator.py``:

* :class:`Aggregator` — frozen pytree dataclass of ``init`` / ``apply`` (:26-53);
* :class:`MeanAggregatorState` — empty state (:56-58);
* :func:`mean_aggregator` — ``apply`` lazily drops client ids and calls
  :func:`fedjax_amd.tree_util.tree_mean` (:61-75; the call at :73), which folds all K clients on
  the GPU in one kernel launch per leaf-dtype group;
* :func:`clipped_mean_aggregator` — the weighted mean of clients each clipped to a maximum
  l2 norm first (the loop of fedjax/algorithms/mime_lite.py:131-149 as an aggregator),
  :func:`fedjax_amd.tree_util.tree_clipped_mean`;
* :func:`dp_clipped_mean_aggregator` — that mean plus Gaussian noise calibrated to the clip norm
  (DP-FedAvg; no reference counterpart), :func:`fedjax_amd.tree_util.tree_dp_clipped_mean`;
* :func:`trimmed_mean_aggregator` / :func:`median_aggregator` — the coordinate-wise trimmed mean
  and median of Yin et al. (ICML 2018; no reference counterpart),
  :func:`fedjax_amd.tree_util.tree_trimmed_mean` / :func:`fedjax_amd.tree_util.tree_median`;
* :func:`krum_aggregator` / :func:`geometric_median_aggregator` — Krum / multi-Krum (Blanchard et
  al., NeurIPS 2017) and the smoothed-Weiszfeld geometric median (Pillutla et al., IEEE TSP 2022;
  no reference counterparts), :func:`fedjax_amd.tree_util.tree_krum` /
  :func:`fedjax_amd.tree_util.tree_geometric_median`;
* :func:`mean_around_median_aggregator` / :func:`bulyan_aggregator` — the mean around the median
  (Xie et al. 2018) and Bulyan (El Mhamdi et al., ICML 2018; no reference counterparts),
  :func:`fedjax_amd.tree_util.tree_mean_around_median` / :func:`fedjax_amd.tree_util.tree_bulyan`;
* :func:`centered_clip_aggregator` — centered clipping around the previous round's aggregate
  (Karimireddy et al., ICML 2021; no reference counterpart), the one aggregator here whose state
  carries the aggregate itself, :func:`fedjax_amd.tree_util.tree_centered_clip`;
* :func:`fltrust_aggregator` — FLTrust's trust-weighted mean against the server's own delta (Cao et
  al., NDSS 2021; no reference counterpart), whose state carries that delta,
  :func:`fedjax_amd.tree_util.tree_fltrust`.
"""

import dataclasses as std_dataclasses
from typing import Any, Callable, Dict, Iterable, Optional, Tuple

import numpy as np

from fedjax_amd import dataclasses
from fedjax_amd import kernels
from fedjax_amd import random as fj_random
from fedjax_amd import tree_util
from fedjax_amd.typing import ClientId, Params

PyTree = Any
AggregatorState = PyTree


@dataclasses.dataclass
class Aggregator:
    """Interface for algorithms to aggregate (aggregator.py:26-53).

    Usage, as in the reference::

      aggregator = mean_aggregator()
      state = aggregator.init()
      for i in range(num_rounds):
        clients_params_and_weights = compute_client_outputs(i)
        aggregated_params, state = aggregator.apply(clients_params_and_weights, state)

    Attributes:
      init: Returns initial state of aggregator.
      apply: Returns the new aggregator state and aggregated params.
    """
    init: Callable[[], AggregatorState]
    apply: Callable[[Iterable[Tuple[ClientId, Params, float]], AggregatorState],
                    Tuple[Params, AggregatorState]]


@dataclasses.dataclass
class MeanAggregatorState:
    """Mean aggregator is stateless."""


def mean_aggregator() -> Aggregator:
    """Builds (weighted) mean aggregator.

    ``apply`` returns ``tree_util.tree_mean``'s result: its float32 leaves may be slices of
    one allocation (see tree_mean), so one kept leaf holds the whole mean's memory."""

    def init():
        return MeanAggregatorState()

    def apply(clients_params_and_weights, state):
        def extract_params_and_weight(clients_params_and_weight):
            _, param, weight = clients_params_and_weight
            return param, weight

        if type(clients_params_and_weights) in (list, tuple) and clients_params_and_weights:
            # resident clients: the triples go to the one-call native path as they are
            # (tree_util.mean_of_triples); a one-shot iterable keeps the lazy map and the
            # streaming fold
            return tree_util.mean_of_triples(clients_params_and_weights), state
        params_and_weights = map(extract_params_and_weight, clients_params_and_weights)
        return tree_util.tree_mean(params_and_weights), state

    return Aggregator(init, apply)


@dataclasses.dataclass
class ClippedMeanAggregatorState:
    """The last round's per-client diagnostics, keyed by client id (0-d device tensors):
    the l2 norm before clipping, the norm after, and whether the client was clipped."""
    norms: Dict[ClientId, Any]
    clipped_norms: Dict[ClientId, Any]
    clipped: Dict[ClientId, Any]
    # dp_clipped_mean_aggregator: the float32 noise standard deviation of the round (else None);
    # a host number, so structure and not a pytree child
    noise_stddev: Optional[float] = std_dataclasses.field(default=None, metadata={"pytree_node": False})


def clipped_mean_aggregator(max_norm: float) -> Aggregator:
    """Builds the (weighted) mean aggregator that clips every client's params to l2 norm
    ``max_norm`` before weighting (tree_clip_by_global_norm, fedjax/core/tree_util.py:117-133,
    as fedjax/algorithms/mime_lite.py:131-149 applies it; the mean divides by the unclipped
    total weight). ``apply`` is :func:`fedjax_amd.tree_util.tree_clipped_mean`: it does not
    synchronise with the host, and the returned state holds the round's diagnostics."""

    def init():
        return ClippedMeanAggregatorState({}, {}, {})

    def apply(clients_params_and_weights, state):
        del state  # each round's diagnostics replace the last round's
        ids, pairs = [], []
        for client_id, param, weight in clients_params_and_weights:
            ids.append(client_id)
            pairs.append((param, weight))
        got = tree_util.tree_clipped_mean(pairs, max_norm)
        if got.norms is None:
            return got.mean, ClippedMeanAggregatorState({}, {}, {})
        return got.mean, ClippedMeanAggregatorState(
            dict(zip(ids, got.norms.unbind())), dict(zip(ids, got.clipped_norms.unbind())),
            dict(zip(ids, got.clipped.unbind())))

    return Aggregator(init, apply)


def dp_noise_stddev(noise_multiplier: float, max_norm: float, weights) -> float:
    """``f32(noise_multiplier * max_norm * max_k(w_k) / W)``, in Python floats: the noise scale
    of a weighted mean whose clients are clipped to ``max_norm``. Replacing one client's update
    moves the clipped weighted mean by at most ``max_norm * w_k / W`` in l2 norm, its
    sensitivity; the Gaussian mechanism's standard deviation is ``noise_multiplier`` times that."""
    ws = [float(tree_util._host_weight(w)) for w in weights]
    W = 0.0
    for w in ws:
        W += w
    return float(np.float32(float(noise_multiplier) * float(max_norm) * max(ws) / W))


def dp_clipped_mean_aggregator(max_norm: float, noise_multiplier: float, rng) -> Aggregator:
    """Builds the differentially private mean aggregator of DP-FedAvg: every client's params are
    clipped to l2 norm ``max_norm`` (as :func:`clipped_mean_aggregator`), averaged by weight, and
    Gaussian noise of standard deviation

        noise_stddev = f32(noise_multiplier * max_norm * max_k(w_k) / W)

    (:func:`dp_noise_stddev`: one client's l2 sensitivity times the multiplier) is added to every
    coordinate, inside the fold (:func:`fedjax_amd.tree_util.tree_dp_clipped_mean`). ``rng`` is a
    :class:`fedjax_amd.random.PRNGSequence` or a key (then a sequence over it): each ``apply``
    takes one fresh key, so no two rounds share noise. The state is a
    :class:`ClippedMeanAggregatorState` with the round's ``noise_stddev``. Privacy accounting is
    the caller's. ``apply`` raises under stream capture (a replay would reuse the noise)."""
    if not isinstance(rng, fj_random.PRNGSequence):
        rng = fj_random.PRNGSequence(fj_random.strict_key(rng))
    for name, v in (("max_norm", max_norm), ("noise_multiplier", noise_multiplier)):
        if not (float(v) >= 0.0 and np.isfinite(float(v))):
            raise ValueError(f"{name} must be finite and >= 0, got {v}")

    def init():
        return ClippedMeanAggregatorState({}, {}, {}, None)

    def apply(clients_params_and_weights, state):
        del state  # each round's diagnostics replace the last round's
        ids, pairs = [], []
        for client_id, param, weight in clients_params_and_weights:
            ids.append(client_id)
            pairs.append((param, weight))
        if not pairs:
            return None, ClippedMeanAggregatorState({}, {}, {}, None)
        stddev = dp_noise_stddev(noise_multiplier, max_norm, [w for _, w in pairs])
        got = tree_util.tree_dp_clipped_mean(pairs, max_norm, stddev, next(rng))
        return got.mean, ClippedMeanAggregatorState(
            dict(zip(ids, got.norms.unbind())), dict(zip(ids, got.clipped_norms.unbind())),
            dict(zip(ids, got.clipped.unbind())), stddev)

    return Aggregator(init, apply)


@dataclasses.dataclass
class RobustAggregatorState:
    """The trimmed-mean and median aggregators are stateless."""


def _bucket_rng(bucket_size, rng):
    """The checked ``(bucket_size, rng)`` of a bucketed aggregator: ``rng`` a
    :class:`fedjax_amd.random.PRNGSequence`, a key (then a sequence over it) or ``None``."""
    if bucket_size is None:
        if rng is not None:
            raise ValueError("rng shuffles the clients of a bucketed aggregator: pass bucket_size too")
        return None, None
    if isinstance(bucket_size, (bool, np.bool_)) or not isinstance(bucket_size, (int, np.integer)):
        raise TypeError(f"bucket_size must be an int >= 1, not {type(bucket_size).__name__}")
    if bucket_size < 1:
        raise ValueError(f"bucket_size must be >= 1, got {bucket_size}")
    if rng is not None and not isinstance(rng, fj_random.PRNGSequence):
        rng = fj_random.PRNGSequence(fj_random.strict_key(rng))
    return int(bucket_size), rng


def trimmed_mean_aggregator(trim, *, bucket_size: Optional[int] = None, rng=None) -> Aggregator:
    """Builds the coordinate-wise trimmed-mean aggregator (Yin et al., ICML 2018): per coordinate
    the ``t`` smallest and ``t`` largest client values are dropped and the rest averaged, in one
    launch (:func:`fedjax_amd.tree_util.tree_trimmed_mean`). ``trim`` is the int count ``t`` or a
    float fraction ``0 <= beta < 0.5`` of the round's clients (``t = floor(beta * K)``).

    ``apply`` takes the usual ``(client_id, params, weight)`` triples and IGNORES the weights: a
    client must not be able to scale its own vote in a robust aggregate. Float32 params, at most
    128 clients a round.

    ``bucket_size=s`` is bucketing (Karimireddy, He and Jaggi, ICLR 2022): each round's clients
    are shuffled, averaged in ``B = ceil(K / s)`` buckets of ``s`` and the rule runs over the
    bucket means; at most 4096 clients and 128 buckets a round. ``rng`` is a
    :class:`fedjax_amd.random.PRNGSequence` or a key (then a sequence over it): each ``apply``
    draws one fresh key and shuffles with :func:`fedjax_amd.random.permutation`, on the device.
    ``rng=None`` buckets consecutive clients, UNSHUFFLED, which the paper's guarantee does not
    cover. ``trim`` and the Byzantine budget now count BUCKETS: ``f`` bad clients can spoil ``f``
    buckets out of ``K / s``, so the fraction of bad clients that a given ``trim`` fraction
    tolerates shrinks by ``s`` (the paper's ``delta * s`` condition)."""
    if isinstance(trim, (bool, np.bool_)) or not isinstance(trim, (int, float, np.integer, np.floating)):
        raise TypeError("trim must be an int count or a float fraction in [0, 0.5)")
    if isinstance(trim, (float, np.floating)) and not (0.0 <= float(trim) < 0.5):
        raise ValueError(f"a trim fraction must be in [0, 0.5), got {trim}")
    if isinstance(trim, (int, np.integer)) and trim < 0:
        raise ValueError(f"a trim count must be >= 0, got {trim}")
    bucket_size, rng = _bucket_rng(bucket_size, rng)

    def init():
        return RobustAggregatorState()

    def apply(clients_params_and_weights, state):
        params = [param for _, param, _ in clients_params_and_weights]  # the weights are not used
        if bucket_size is None or not params:
            return tree_util.tree_trimmed_mean(params, trim, bucket_size=bucket_size), state
        kernels.bucket_count(len(params), bucket_size)  # refuse the round before a key is drawn
        perm = None if rng is None else fj_random.permutation(next(rng), len(params))
        return tree_util.tree_trimmed_mean(params, trim, bucket_size=bucket_size, perm=perm), state

    return Aggregator(init, apply)


def median_aggregator(*, bucket_size: Optional[int] = None, rng=None) -> Aggregator:
    """Builds the coordinate-wise median aggregator (Yin et al., ICML 2018):
    :func:`fedjax_amd.tree_util.tree_median` of the round's params. ``apply`` takes the usual
    triples and IGNORES the weights. Float32 params, at most 128 clients a round.

    ``bucket_size`` and ``rng`` as :func:`trimmed_mean_aggregator` takes them: the median of the
    means of shuffled buckets of ``bucket_size`` clients, for up to 4096 clients a round;
    ``rng=None`` buckets consecutive clients, UNSHUFFLED. The Byzantine budget counts BUCKETS:
    the median tolerates fewer than half the buckets spoiled, so fewer than ``K / (2 s)`` bad
    clients (the paper's ``delta * s`` condition)."""
    bucket_size, rng = _bucket_rng(bucket_size, rng)

    def init():
        return RobustAggregatorState()

    def apply(clients_params_and_weights, state):
        params = [param for _, param, _ in clients_params_and_weights]  # the weights are not used
        if bucket_size is None or not params:
            return tree_util.tree_median(params, bucket_size=bucket_size), state
        kernels.bucket_count(len(params), bucket_size)  # refuse the round before a key is drawn
        perm = None if rng is None else fj_random.permutation(next(rng), len(params))
        return tree_util.tree_median(params, bucket_size=bucket_size, perm=perm), state

    return Aggregator(init, apply)


@dataclasses.dataclass
class KrumAggregatorState:
    """The last round's selection: ``selected`` — the client ids Krum chose, best first;
    ``scores`` — every client's Krum score by client id (float; ``inf`` for a client whose
    params held a non-finite value). Empty before the first round."""
    selected: Tuple[ClientId, ...] = ()
    scores: Dict[ClientId, float] = std_dataclasses.field(default_factory=dict)


@dataclasses.dataclass
class DeviceKrumAggregatorState:
    """The last round's selection with ``select="device"``, still on the device: ``client_ids`` —
    the round's ids in client order; ``selected`` — int64 device tensor of indices into them,
    best first, -1 padded; ``count`` — int32 device scalar, how many were selected; ``scores`` —
    float64 device tensor, one per client. Reading any of them is the caller's synchronisation."""
    client_ids: Tuple[ClientId, ...] = ()
    selected: Any = None
    count: Any = None
    scores: Any = None


def krum_aggregator(num_byzantine: int, num_selected: int = 1, *, select: str = "host") -> Aggregator:
    """Builds the Krum (``num_selected = 1``) / multi-Krum aggregator of Blanchard et al.
    (NeurIPS 2017): :func:`fedjax_amd.tree_util.tree_krum` of the round's params — the mean of
    the ``num_selected`` clients closest to their ``K - num_byzantine - 2`` nearest neighbours.
    A round needs ``K >= 2 * num_byzantine + 3`` clients.

    ``apply`` takes the usual ``(client_id, params, weight)`` triples and IGNORES the weights: a
    client must not be able to scale its own vote. It returns ``None`` for a round with no
    clients or no selectable client. Float32 params, at most 1024 clients a round.

    ``select="device"`` runs the selection on the device (``tree_krum(..., select="device")``): no
    host step between the two passes. The mean of a round without a selectable client is then all
    +0 instead of ``None``, and the state is a :class:`DeviceKrumAggregatorState` of device
    tensors."""
    device = kernels.check_select(select)
    if isinstance(num_byzantine, (bool, np.bool_)) or not isinstance(num_byzantine, (int, np.integer)):
        raise TypeError("num_byzantine must be an int")
    if isinstance(num_selected, (bool, np.bool_)) or not isinstance(num_selected, (int, np.integer)):
        raise TypeError("num_selected must be an int")
    if num_byzantine < 0 or num_selected < 1:
        raise ValueError(f"need num_byzantine >= 0 and num_selected >= 1, got {num_byzantine} and {num_selected}")

    def init():
        return KrumAggregatorState()

    def apply(clients_params_and_weights, state):
        triples = list(clients_params_and_weights)  # the weights are not used
        if device:
            got = tree_util.tree_krum([param for _, param, _ in triples], num_byzantine, num_selected,
                                      select="device")
            if got is None:
                return None, DeviceKrumAggregatorState()
            return got.mean, DeviceKrumAggregatorState(tuple(cid for cid, _, _ in triples), got.selected,
                                                       got.count, got.scores)
        got = tree_util.tree_krum([param for _, param, _ in triples], num_byzantine, num_selected)
        if got is None:
            return None, KrumAggregatorState()
        ids = [cid for cid, _, _ in triples]
        return got.mean, KrumAggregatorState(tuple(ids[k] for k in got.selected),
                                            {cid: float(s) for cid, s in zip(ids, got.scores)})

    return Aggregator(init, apply)


def mean_around_median_aggregator(keep: int) -> Aggregator:
    """Builds the mean-around-the-median aggregator ("MeaMed", Xie et al. 2018): per coordinate
    the mean of the ``keep`` client values closest to the coordinate's median, in one launch
    (:func:`fedjax_amd.tree_util.tree_mean_around_median`). A round needs ``K >= keep`` clients.

    ``apply`` takes the usual ``(client_id, params, weight)`` triples and IGNORES the weights: a
    client must not be able to scale its own vote in a robust aggregate. Float32 params, at most
    128 clients a round."""
    if isinstance(keep, (bool, np.bool_)) or not isinstance(keep, (int, np.integer)):
        raise TypeError("keep must be an int count")
    if keep < 1:
        raise ValueError(f"a keep count must be >= 1, got {keep}")

    def init():
        return RobustAggregatorState()

    def apply(clients_params_and_weights, state):
        params = [param for _, param, _ in clients_params_and_weights]  # the weights are not used
        return tree_util.tree_mean_around_median(params, keep), state

    return Aggregator(init, apply)


@dataclasses.dataclass
class BulyanAggregatorState:
    """The last round's selection: ``selected`` — the client ids Bulyan's first stage chose, in
    selection order; ``keep`` — how many of their values the second stage averaged per
    coordinate. Empty before the first round."""
    selected: Tuple[ClientId, ...] = ()
    keep: int = 0


@dataclasses.dataclass
class DeviceBulyanAggregatorState:
    """The last round's selection with ``select="device"``, still on the device: ``client_ids`` —
    the round's ids in client order; ``selected`` — int64 device tensor of indices into them, in
    selection order, -1 padded; ``count`` — int32 device scalar, how many were selected; ``keep`` —
    int32 device scalar, how many values the second stage averaged per coordinate (0: no mean).
    Reading any of them is the caller's synchronisation."""
    client_ids: Tuple[ClientId, ...] = ()
    selected: Any = None
    count: Any = None
    keep: Any = None


def bulyan_aggregator(num_byzantine: int, *, select: str = "host") -> Aggregator:
    """Builds the Bulyan aggregator of El Mhamdi, Guerraoui and Rouault (ICML 2018):
    :func:`fedjax_amd.tree_util.tree_bulyan` of the round's params — ``K - 2f`` clients chosen by
    iterated Krum, ``f = num_byzantine``, then per coordinate the mean of the ``K - 4f`` chosen
    values closest to their median. A round needs ``K >= 4f + 3`` clients.

    ``apply`` takes the usual ``(client_id, params, weight)`` triples and IGNORES the weights: a
    client must not be able to scale its own vote. It returns ``None`` for a round with no
    clients or too few selectable ones. Float32 params, at most 1024 clients a round with
    ``K - 2f <= 128``.

    ``select="device"`` runs the selection on the device (``tree_bulyan(..., select="device")``): no
    host step between the two passes. The mean of a round with too few selectable clients is then
    all +0 instead of ``None``, and the state is a :class:`DeviceBulyanAggregatorState` of device
    tensors."""
    device = kernels.check_select(select)
    if isinstance(num_byzantine, (bool, np.bool_)) or not isinstance(num_byzantine, (int, np.integer)):
        raise TypeError("num_byzantine must be an int")
    if num_byzantine < 0:
        raise ValueError(f"need num_byzantine >= 0, got {num_byzantine}")

    def init():
        return BulyanAggregatorState()

    def apply(clients_params_and_weights, state):
        triples = list(clients_params_and_weights)  # the weights are not used
        if device:
            got = tree_util.tree_bulyan([param for _, param, _ in triples], num_byzantine, select="device")
            if got is None:
                return None, DeviceBulyanAggregatorState()
            return got.mean, DeviceBulyanAggregatorState(tuple(cid for cid, _, _ in triples), got.selected,
                                                         got.count, got.keep)
        got = tree_util.tree_bulyan([param for _, param, _ in triples], num_byzantine)
        if got is None:
            return None, BulyanAggregatorState()
        ids = [cid for cid, _, _ in triples]
        return got.mean, BulyanAggregatorState(tuple(ids[k] for k in got.selected), int(got.keep))

    return Aggregator(init, apply)


@dataclasses.dataclass
class GeometricMedianAggregatorState:
    """The last round's Weiszfeld weight per client id (float32 as the fold used it; 0 for a
    client whose params held a non-finite value). Empty before the first round."""
    weights: Dict[ClientId, float] = std_dataclasses.field(default_factory=dict)


@dataclasses.dataclass
class DeviceGeometricMedianAggregatorState:
    """The last round's Weiszfeld weights with ``select="device"``, still on the device:
    ``client_ids`` — the round's ids in client order; ``weights`` — float32 device tensor, one per
    client (0 for an unusable one); ``count`` — int32 device scalar, the clients with a positive
    weight."""
    client_ids: Tuple[ClientId, ...] = ()
    weights: Any = None
    count: Any = None


def geometric_median_aggregator(iterations: int = 4, nu: float = 1e-6, *, select: str = "host") -> Aggregator:
    """Builds the geometric-median aggregator ("RFA", Pillutla et al., IEEE TSP 2022):
    :func:`fedjax_amd.tree_util.tree_geometric_median` of the round's params with unit client
    weights, ``iterations`` smoothed Weiszfeld steps with smoothing ``nu``.

    ``apply`` takes the usual triples and IGNORES the weights. It returns ``None`` for a round
    with no clients or no usable client. Float32 params, at most 1024 clients a round.

    ``select="device"`` runs the iteration on the device
    (``tree_geometric_median(..., select="device")``): no host step between the two passes. The
    median of a round without a usable client is then all +0 instead of ``None``, and the state is
    a :class:`DeviceGeometricMedianAggregatorState` of device tensors."""
    device = kernels.check_select(select)
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)):
        raise TypeError("iterations must be an int")
    if iterations < 0:
        raise ValueError(f"iterations must be >= 0, got {iterations}")
    if isinstance(nu, (bool, np.bool_)) or not isinstance(nu, (int, float, np.integer, np.floating)):
        raise TypeError("nu must be a number")
    if not (float(nu) > 0.0 and np.isfinite(float(nu))):
        raise ValueError(f"nu must be finite and > 0, got {nu}")

    def init():
        return GeometricMedianAggregatorState()

    def apply(clients_params_and_weights, state):
        triples = list(clients_params_and_weights)  # the weights are not used
        if device:
            got = tree_util.tree_geometric_median([param for _, param, _ in triples], iterations=iterations, nu=nu,
                                                  select="device")
            if got is None:
                return None, DeviceGeometricMedianAggregatorState()
            return got.median, DeviceGeometricMedianAggregatorState(tuple(cid for cid, _, _ in triples),
                                                                    got.weights, got.count)
        got = tree_util.tree_geometric_median([param for _, param, _ in triples], iterations=iterations, nu=nu)
        if got is None:
            return None, GeometricMedianAggregatorState()
        return got.median, GeometricMedianAggregatorState(
            {cid: float(w) for (cid, _, _), w in zip(triples, got.weights)})

    return Aggregator(init, apply)


@dataclasses.dataclass
class CenteredClipAggregatorState:
    """What centered clipping carries from round to round: ``center`` — the last round's
    aggregate (``None`` before the first round, which clips around zeros), the SAME tensors
    ``apply`` returned, not a copy: whoever writes into the returned aggregate moves the next
    round's centre; ``distances`` / ``factors`` — by client id, the last iteration's l2 distance
    of the client from the centre and its clip factor (0-d device tensors; NaN / 0 for a client
    that was skipped)."""
    center: Any = None
    distances: Dict[ClientId, Any] = std_dataclasses.field(default_factory=dict)
    factors: Dict[ClientId, Any] = std_dataclasses.field(default_factory=dict)


def centered_clip_aggregator(tau: float, iterations: int = 1) -> Aggregator:
    """Builds the centered-clipping aggregator of Karimireddy, He and Jaggi (ICML 2021; no reference
    counterpart): every client's params are clipped to l2 distance ``tau`` from the previous
    round's aggregate and averaged around it, ``iterations`` times
    (:func:`fedjax_amd.tree_util.tree_centered_clip`). The state is the history the rule needs:
    ``apply`` clips around ``state.center`` (zeros in the first round), returns the new centre as
    the aggregate and keeps those same tensors in the new state.

    ``apply`` takes the usual ``(client_id, params, weight)`` triples and IGNORES the weights: a
    client must not be able to scale its own vote in a robust aggregate. A round with no clients
    returns ``None`` and leaves the state as it was. Float32 params, at most 4096 clients a round;
    no host synchronisation."""
    kernels.check_center_args(1, tau, iterations)

    def init():
        return CenteredClipAggregatorState()

    def apply(clients_params_and_weights, state):
        ids, params = [], []
        for client_id, param, _ in clients_params_and_weights:  # the weights are not used
            ids.append(client_id)
            params.append(param)
        got = tree_util.tree_centered_clip(params, tau, None if state is None else state.center,
                                           iterations=iterations)
        if got is None:
            return None, state
        return got.center, CenteredClipAggregatorState(
            got.center, dict(zip(ids, got.distances[-1].unbind())), dict(zip(ids, got.factors[-1].unbind())))

    return Aggregator(init, apply)


@dataclasses.dataclass
class FLTrustAggregatorState:
    """What FLTrust needs beside the clients and what it reports: ``server_delta`` — the delta the
    server computed itself on its trusted dataset for THIS round, a pytree of the clients'
    structure; the caller sets it before every ``apply`` with ``state.replace(server_delta=...)``
    (``None``: ``apply`` raises); ``trust`` / ``factors`` — by client id, the last round's trust
    score ``ts_k`` (float64) and rescale factor ``c_k`` (float32) as 0-d device tensors (0 for a
    client that was gated out and never loaded by the fold)."""
    server_delta: Any = None
    trust: Dict[ClientId, Any] = std_dataclasses.field(default_factory=dict)
    factors: Dict[ClientId, Any] = std_dataclasses.field(default_factory=dict)


def fltrust_aggregator() -> Aggregator:
    """Builds the FLTrust aggregator of Cao, Fang, Liu and Gong (NDSS 2021; no reference
    counterpart): every client's params are weighed by the ReLU of their cosine with the server's
    own delta, rescaled to that delta's norm and averaged by trust
    (:func:`fedjax_amd.tree_util.tree_fltrust`). The rule judges a client against the server, not
    against the other clients, so it needs no honest majority — and it needs the server's delta:
    ``state.server_delta`` must be set for every round (``state.replace(server_delta=g)``);
    ``apply`` raises ``ValueError`` while it is ``None`` and carries it over unchanged.

    ``apply`` takes the usual ``(client_id, params, weight)`` triples and IGNORES the weights: a
    client must not be able to scale its own vote in a robust aggregate. A round with no clients
    returns ``None`` and leaves the state as it was; a round that trusts nobody returns all +0.
    Float32 params, at most 4096 clients a round; no host synchronisation."""

    def init():
        return FLTrustAggregatorState()

    def apply(clients_params_and_weights, state):
        if state is None or state.server_delta is None:
            raise ValueError("fltrust_aggregator: set state.server_delta (the server's own delta of this round) "
                             "with state.replace(server_delta=...) before apply")
        ids, params = [], []
        for client_id, param, _ in clients_params_and_weights:  # the weights are not used
            ids.append(client_id)
            params.append(param)
        got = tree_util.tree_fltrust(params, state.server_delta)
        if got is None:
            return None, state
        return got.mean, FLTrustAggregatorState(state.server_delta, dict(zip(ids, got.trust.unbind())),
                                                dict(zip(ids, got.factors.unbind())))

    return Aggregator(init, apply)
