"""Square attack on the object patch: the black-box random search from the literature (Andriushchenko et al., "Square Attack",
arXiv:1912.00049) in the reference's ``evaluate_attacks`` (``MD2/evaluate_depth.py:142-145``, ``norm_type == "Square"``).

Same class name, constructor, call signature and return tuple as the reference's ``torchattacks/attacks/phy_obj_atk_square.py``
(forward :83-121, attack_single_run :251-329).  Unlike the tube-light and Gaussian-blur rows the candidate depends on the model's
earlier answers -- ``x_best`` evolves -- but every random draw does not: the start stripes and per iteration (vh, vw, signs) come
from the CPU torch generator, and the poses from ``np.random.RandomState(seed)``, made afresh in every ``depth_loss`` call, so
every query pastes at the SAME poses.  All draws are made on the host before the first launch, in the reference's order, and the
loop reads nothing back:

    per query   K27 square_propose (x_best <- x_new if the previous query became the best; x_new <- the next candidate)
                -> K3 eot_paste -> model / K19 windowed cost -> K24 tube_light_commit (cost array, best cost, best query, cursor)

with ONE window plan, one clean-frame paste and one coefficient row for the whole search.  After the loop one absorb-only
propose takes in the last decision, and the cost array and the best index are read once.

What the reference's code really does (``norm='Linf'``; its ``L2`` branch calls ``margin_and_loss`` with an undefined ``y``):
``margin`` is ``ones(1)``, so the loop never leaves early and ``n_restarts > 1`` does nothing after the first restart; and :295
evaluates ``depth_loss(x_best, ...)`` instead of auto-attack's ``x_new`` (the commented line :294).  With fixed poses and a
deterministic model every query then returns the first cost, ``loss < loss_min`` is never true, and the result is the start
stripes after ``n_queries`` wasted model calls.  ``query_patch="best"`` is that line; the default ``"candidate"`` evaluates
``x_new``, the algorithm of the paper.  Both go through the same kernels and differ only in which buffer is pasted.

One more difference, kept knowingly: after a NaN cost the reference's ``loss_min`` itself turns NaN (``0 * nan`` in :300-301) and
no later query is accepted; here K24's strict comparison rejects the NaN query and the search goes on from the best so far.
"""
import numpy as np
import torch

from ... import ops
from ...my_utils import to_device_async
from .object_search import _ObjectSearch


class Phy_obj_atk_Square(_ObjectSearch):
    r"""
    Distance Measure : Linf

    Arguments:
        model (nn.Module): model to attack.
        obj_img (1xCxHxW), obj_mask (1x1xHxW): object patch and its paint mask.
        norm (str): only 'Linf' (the reference's 'L2' branch cannot run). (Default: 'Linf')
        eps (float): maximum perturbation. (Default: 0.1)
        n_queries (int): iterations of the search; with the start point the model is asked n_queries + 1 times. (Default: 5000)
        p_init (float): fraction of the object the first squares cover. (Default: 0.8)
        resc_schedule (bool): adapt the schedule of p to n_queries. (Default: True)
        seed (int): seed of the poses' ``np.random.RandomState``. (Default: 0)
        n_restarts, loss, verbose: accepted as the reference accepts them; inert there (see the module text) and here.
        query_patch ("candidate" | "best"): which patch a query pastes; "best" is the reference's line :295.
        host_chain (bool): run the reference's shape instead -- the candidate in torch on the host, an upload and a host
            comparison per query -- on the same paste / cost kernels (the benchmark's baseline and the tests' eager twin).

    ``use_graph`` (attribute, off by default): queries 0 and 1 run eagerly, query 2 is captured in a HIP graph and replayed for
    the rest; a failed capture hands the search back to the eager loop with ``graph_failure`` set.
    """

    shared_poses = True

    def __init__(self, model, obj_img, obj_mask, norm='Linf', eps=0.1, n_queries=5000, n_restarts=1, p_init=.8, loss='margin',
                 resc_schedule=True, seed=0, verbose=False, dist_range=list(range(5, 31, 2)), query_patch="candidate",
                 host_chain=False):
        if norm != 'Linf':
            raise NotImplementedError("Phy_obj_atk_Square: norm %r is not built (the reference's L2 branch cannot run: it calls "
                                      "margin_and_loss with an undefined y)" % (norm,))
        if eps is None:
            raise ValueError("Phy_obj_atk_Square: eps must be given")
        if int(n_queries) < 1:
            raise ValueError("Phy_obj_atk_Square: n_queries must be positive")
        if query_patch not in ("candidate", "best"):
            raise ValueError("Phy_obj_atk_Square: query_patch must be 'candidate' or 'best'")
        super().__init__(model, obj_img, obj_mask, host_chain=host_chain, eps=eps, dist_range=dist_range)
        self.attack = "Square"
        self.norm, self.n_queries, self.p_init, self.n_restarts, self.seed = norm, int(n_queries), p_init, n_restarts, seed
        self.verbose, self.loss, self.rescale_schedule, self.query_patch = verbose, loss, resc_schedule, query_patch
        self.accepted = None        # after the search: the queries that became the best, in order (query 0 = the stripes)
        self.graph_replays = 0
        self._x_best = None
        # trace (see _ObjectSearch): square = (vh, vw, s) and signs, None for the stripes.  _capture_fault makes the capture
        # of the query fail before its first launch.

    # ------------------------------------------------------------------------------------------------------------- the draws
    def _prepare(self, obj):
        """The CPU torch generator's stream first (:259-260, :282-286), as the reference draws it; a schedule with a square larger
        than the object is refused here, before the pose draws."""
        c, h, w = (int(v) for v in obj.shape[-3:])
        try:
            table, stripes = ops.square_table(self.n_queries, c, h, w, self.p_init, self.rescale_schedule)
        except RuntimeError as e:
            raise ValueError("Phy_obj_atk_Square: " + str(e))
        return len(table), (table, stripes)

    def _pose_draws(self, batch_size, n):
        """:126: the one pose set of every depth_loss call."""
        return [self.phy_trans_ben.draw_samples(batch_size, rs=np.random.RandomState(self.seed))]

    # ------------------------------------------------------------------------------------------------------- the device loop
    def _device_search(self, obj, n, ctx):
        table_host, stripes_host = ctx
        table, stripes = to_device_async(table_host, self.device), to_device_async(stripes_host, self.device)
        self._x_best = obj.clone()
        eps = float(self.eps)
        return ops.tube_light_state(n, self.device), \
            lambda state, out: ops.square_propose(obj, self._x_best, out, table, stripes, state, eps)

    def _pasted(self, q, patch):
        return self._x_best if self.query_patch == "best" and q > 0 else patch

    def _run_queries(self, n, query):
        done = 0
        self.graph_replays = 0
        if self.use_graph and n >= 4 and self.device.type == "cuda" and not ops.profiling_every_launch():
            query(0)        # the stripes: with the warm-up pass it has filled every cache of the frozen-weights scope
            query(1)
            done = 2

            def traced():
                if self._capture_fault:     # test hook: a capture that dies before its first launch
                    raise RuntimeError("injected capture fault")
                query(2)

            # every buffer a query updates is updated in place (K27, K24), and poses and windows never move: a replay IS the
            # next query, and after a failed capture the eager loop goes on from the state query 1 left
            g = self._capture_graph(traced, what="the query", restore_head=True)
            if g is not None:
                for _ in range(2, n):
                    g.replay()
                self.graph_replays = n - 2
                done = n
                self._keep_graph(g)
        for q in range(done, n):
            query(q)

    def _finish(self, compose, state, patch, adv_patch):
        compose(state, patch)       # the cursor stands at n: absorb the last decision, make no candidate
        adv_patch.copy_(self._x_best)
        self._x_best = None

    def _record(self, costs, best):
        """The accepted queries from the cost array's running strict minimum (K24's rule: below 1e10, a NaN never)."""
        low, self.accepted = np.float32(1e10), []
        for q, c in enumerate(np.asarray(costs, dtype=np.float32)):
            if c < low:
                low = c
                self.accepted.append(q)
        if (self.accepted[-1] if self.accepted else -1) != best:
            raise RuntimeError("Phy_obj_atk_Square: the cost array and the device's best query disagree (%r, %d)"
                               % (self.accepted, best))

    # ---------------------------------------------------------------------------------------------------------- the host chain
    def _host_search(self, obj, n, ctx, cost_of, adv_patch):
        """The reference's loop shape on this project's paste and cost: the candidate in torch on the host, one upload and one
        host comparison per query.  Returns (costs, best query); ``adv_patch`` receives x_best."""
        table, stripes = ctx
        x0 = obj.cpu()
        x_best, x_new = x0.clone(), torch.zeros_like(x0)
        eps = float(self.eps)
        costs = np.zeros(n, dtype=np.float32)
        best_cost, best = 1e10, -1
        with torch.no_grad():
            cost_of(obj, 0)         # the same warm-up as the device loop's
        with torch.no_grad(), self.loop_context():
            for q in range(n):
                x_best, x_new = ops.square_host(x0, x_best, x_new, table, stripes, q, q > 0 and best == q - 1, eps)
                pasted = x_best if self.query_patch == "best" and q > 0 else x_new
                cost = cost_of(pasted.to(self.device).contiguous(), q)
                if cost < best_cost:        # the reference's host read (:298)
                    best_cost, best = cost, q
                costs[q] = float(cost)
        x_best, _ = ops.square_host(x0, x_best, x_new, table, stripes, n, best == n - 1, eps)
        adv_patch.copy_(x_best)
        return costs, best

    def _trace_fields(self, ctx, q):
        row = ctx[0][q]
        if q == 0:
            return dict(square=None, signs=None)
        return dict(square=tuple(int(v) for v in row[:3]), signs=tuple(int(v) for v in row[3:]))
