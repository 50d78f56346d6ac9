"""Float64 / integer oracle of the stored-state refresh (csrc/kernels/state_refresh.hip,
``replay.state_refresh``): which recurrent states of a learner step go back into the replay, who
writes a row that several batch slots reach, and how far the stored states had drifted.

Pure host code (numpy, no torch, no GPU).  tests/test_state_refresh_cpu.py checks it against a
brute-force simulation and shows that the checks reject wrong variants; tests/test_state_refresh_gpu.py
runs the kernel and the engine through it.

The rule.  Batch slot b starts at row s_b; R(b, j) = ring_row(s_b, j) wraps inside the slot's own
sub-ring; T = burn_in + learn.  Chain c ("on": online net, "tg": target net; the online-on-next chain
"nx" is never a source) consumed at its step t the frame of row R(b, o_c + t) and produced (h_t, c_t),
with o_on = 0 and o_tg = 0 ("shifted") or n_step ("fixed", "reference").

* row offset: the state of step t belongs to row offset j = o_c + t with stored_state "post" (the
  state after consuming that row's frame, the reference's convention) and j = o_c + t + 1 with "pre"
  (the state before it) -- the switch of actor_batched._args (h32_new / h32).
* eligibility: (b, c, t) is eligible iff t >= context and j <= T - 1.  The bootstrap rows T .. T+n-1
  may belong to the next episode and are never written.
* ownership: of the eligible entries of one net that reach the same physical row, the one with the
  largest t writes it (the most context); ties go to the smallest b.  Each row is written once.
* value: c is the chain's fp32 cell state; h is float(hi) + float(lo), one fp32 add, in split
  precision and float(bf16) in the bf16 engine.  Online states go to hs_cs, target-chain states to
  target_hs_cs.
* drift: over the owned rows only, per net and for h and c apart, sum (new - old)^2 and sum new^2,
  plus the row count; "measure" computes them and writes nothing, "write" computes them from the
  values it overwrites.

Bound of the drift sums (u = 2^-24, derived here, not fitted to a run).  The kernel forms d =
fl(new - old) (one rounding, relative u), then fma(d, d, acc) and fma(new, new, acc): a sum of N
non-negative fp32 terms, each carrying at most (1 + u)^2, added in some fixed order with one
rounding per addition.  Whatever the order, no term passes through more than N - 1 additions, so the
result is within gamma(N + 1) = (N + 1) u / (1 - (N + 1) u) of the float64 sum, relative.  N is the
term count, rows x H.  The row count is an integer and exact.

``mutation`` (tests only): a deliberately wrong variant of one rule; ``MUTATIONS`` lists them.
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import numpy as np

from .refnum import bf16_val
from .replay_ref import ring_row

MUTATIONS = ("j_off_by_one", "tie_larger_b", "bootstrap_rows", "drift_double_count")
MODES = ("off", "measure", "write")
CHAINS = ("on", "tg")
U24 = 2.0 ** -24


class Spec(NamedTuple):
    B: int
    burn_in: int
    learn: int
    n_step: int
    cap_e: int
    target_mode: str = "shifted"     # shifted | fixed | reference
    stored_state: str = "post"       # post | pre
    context: int = -1                # -1: burn_in

    @property
    def T(self) -> int:
        return self.burn_in + self.learn

    @property
    def ctx(self) -> int:
        return self.burn_in if self.context < 0 else int(self.context)


def check_config(mode: str, context: int, burn_in: int, learn: int) -> int:
    """The knobs' own refusals (the engine adds its own); returns the resolved context."""
    if mode not in MODES:
        raise ValueError(f"replay.state_refresh must be one of {MODES}, not {mode!r}")
    T = burn_in + learn
    ctx = burn_in if int(context) < 0 else int(context)
    if int(context) < -1 or not 0 <= ctx <= T - 1:
        raise ValueError(f"replay.state_refresh_context = {context}: a recomputed state has between 0 "
                         f"and burn_in + learn - 1 = {T - 1} chain steps behind it (-1: burn_in)")
    return ctx


def chain_offset(chain: str, target_mode: str, n_step: int) -> int:
    """o_c: the row offset of the first frame chain ``chain`` consumes."""
    if chain == "on":
        return 0
    if chain != "tg":
        raise ValueError(f"chain {chain!r} is not a source of refreshed states")
    if target_mode not in ("shifted", "fixed", "reference"):
        raise ValueError(f"unknown target_mode {target_mode!r}")
    return 0 if target_mode == "shifted" else int(n_step)


def row_shift(stored_state: str) -> int:
    if stored_state not in ("post", "pre"):
        raise ValueError(f"unknown stored_state {stored_state!r}")
    return 1 if stored_state == "pre" else 0


def step_range(spec: Spec, chain: str, mutation: Optional[str] = None):
    """(t_lo, t_hi, j - t): the eligible chain steps t_lo .. t_hi (inclusive; empty when t_hi <
    t_lo) and the row offset of step t minus t."""
    dj = chain_offset(chain, spec.target_mode, spec.n_step) + row_shift(spec.stored_state)
    if mutation == "j_off_by_one":
        dj += 1
    j_hi = spec.T - 1
    if mutation == "bootstrap_rows":
        j_hi = spec.T + spec.n_step - 1
    return spec.ctx, j_hi - dj, dj


class Owners(NamedTuple):
    rows: np.ndarray    # distinct physical rows, ascending
    b: np.ndarray       # the owning slot of each
    t: np.ndarray       # its chain step


def entries(starts, spec: Spec, chain: str, mutation: Optional[str] = None):
    """(rows, b, t) of every eligible entry of one net, slot-major."""
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    assert starts.size == spec.B
    t_lo, t_hi, dj = step_range(spec, chain, mutation)
    ts = np.arange(t_lo, max(t_hi, t_lo - 1) + 1, dtype=np.int64)
    b = np.repeat(np.arange(spec.B, dtype=np.int64), ts.size)
    t = np.tile(ts, spec.B)
    return ring_row(starts[b], t + dj, spec.cap_e), b, t


def owners(starts, spec: Spec, chain: str, mutation: Optional[str] = None) -> Owners:
    """One owner per physical row: sort the entries by (row, t descending, b ascending) and keep
    the first of each row."""
    rows, b, t = entries(starts, spec, chain, mutation)
    kb = -b if mutation == "tie_larger_b" else b
    order = np.lexsort((kb, -t, rows))
    rows, b, t = rows[order], b[order], t[order]
    first = np.ones(rows.size, dtype=bool)
    first[1:] = rows[1:] != rows[:-1]
    return Owners(rows[first], b[first], t[first])


def combine_h(hi, lo=None) -> np.ndarray:
    """The fp32 h of a chain: ``hi`` / ``lo`` are bf16 bit patterns (uint16) or fp32 values that
    are exact in bf16; split precision adds the planes with one fp32 add."""
    def val(x):
        x = np.asarray(x)
        return bf16_val(x) if x.dtype == np.uint16 else x.astype(np.float32)
    h = val(hi)
    return h if lo is None else (h + val(lo)).astype(np.float32)


class Refresh(NamedTuple):
    hs_cs: np.ndarray              # (cap, 2H) fp32 after the launch
    target_hs_cs: np.ndarray
    owners: Dict[str, Owners]
    sums: Dict[str, np.ndarray]    # per chain float64 [sum dh^2, sum h^2, sum dc^2, sum c^2]
    rows: Dict[str, int]           # per chain: rows refreshed


def refresh_ref(starts, spec: Spec, h, c, hs_cs, target_hs_cs, mode: str = "write",
                mutation: Optional[str] = None) -> Refresh:
    """``h`` / ``c``: per chain the fp32 (steps, B, H) states (``combine_h`` for h).  ``hs_cs`` /
    ``target_hs_cs``: (cap, 2H) fp32 [h | c] before the launch."""
    if mode not in ("measure", "write"):
        raise ValueError("refresh_ref runs the modes that launch: measure, write")
    out = {"on": np.array(hs_cs, dtype=np.float32), "tg": np.array(target_hs_cs, dtype=np.float32)}
    own, sums, nrows = {}, {}, {}
    for ch in CHAINS:
        hh, cc = np.asarray(h[ch], np.float32), np.asarray(c[ch], np.float32)
        H = hh.shape[-1]
        o = owners(starts, spec, ch, mutation)
        if mutation == "drift_double_count":      # every eligible entry, not the owners alone
            o = Owners(*entries(starts, spec, ch))
        own[ch] = o
        assert o.t.size == 0 or int(o.t.max()) < hh.shape[0], "a chain is shorter than its eligible steps"
        new = np.concatenate([hh[o.t, o.b], cc[o.t, o.b]], axis=1).reshape(-1, 2 * H)
        old = out[ch][o.rows].astype(np.float64)
        d2, n2 = (new.astype(np.float64) - old) ** 2, new.astype(np.float64) ** 2
        sums[ch] = np.array([d2[:, :H].sum(), n2[:, :H].sum(), d2[:, H:].sum(), n2[:, H:].sum()])
        nrows[ch] = int(o.rows.size)
        if mode == "write":
            out[ch][o.rows] = new
    return Refresh(out["on"], out["tg"], own, sums, nrows)


def drift_bound(n_terms: int) -> float:
    """Relative bound of an fp32 drift sum of ``n_terms`` terms (module docstring)."""
    k = (int(n_terms) + 1) * U24
    return k / (1.0 - k)


def check_drift(ref: Refresh, H: int, got_sums, got_rows) -> float:
    """``got_sums``: per chain the kernel's four fp32 sums; ``got_rows``: per chain its row count.
    Returns the largest share of the bound used."""
    worst = 0.0
    for ch in CHAINS:
        assert int(got_rows[ch]) == ref.rows[ch], f"{ch}: {int(got_rows[ch])} rows, oracle {ref.rows[ch]}"
        g = np.asarray(got_sums[ch], dtype=np.float64).reshape(4)
        want = ref.sums[ch]
        bound = drift_bound(ref.rows[ch] * H) * want
        err = np.abs(g - want)
        assert np.isfinite(g).all() and (err <= bound).all(), \
            f"{ch}: drift sums {g} vs oracle {want} (bound {bound})"
        pos = bound > 0
        if pos.any():
            worst = max(worst, float((err[pos] / bound[pos]).max()))
    return worst


def drift_ratio(sums) -> Dict[str, float]:
    """sqrt(sum diff^2 / sum new^2) for h and c from one chain's four sums (0 when nothing was new)."""
    s = np.asarray(sums, dtype=np.float64).reshape(4)
    r = lambda a, b: float(np.sqrt(a / b)) if b > 0 else 0.0   # noqa: E731
    return {"h": r(s[0], s[1]), "c": r(s[2], s[3])}
