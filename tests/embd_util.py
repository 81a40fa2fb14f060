"""Embedding reference for the tests: result_norm rows of the CPU oracle -- the residual stream
after the last layer through the final norm, the vector the oracle hands to its output head -- and
their pooled forms (llama.cpp b5187 build_pooling).

The oracles (ggml_ref.LlamaOracle, cvec_util.CvecOracle, lora_util.LoraOracle) are not copied: for
the length of a call EmbdTap wraps ggml_ref.mul_mat_vec and records the `x` of the call whose `raw`
is the output tensor's data, which every oracle makes once per token with the final-normed vector.
It also wraps rms_norm / layer_norm to keep that norm's input (the pre-norm residual) and its
unweighted output: the wrong references of the power checks."""
import numpy as np

import cvec_util
import ggml_ref as R
import util


def _addr(a):
    a = np.asarray(a)
    return a.__array_interface__["data"][0], a.nbytes


class EmbdTap:
    """with EmbdTap(head) as tap: ... oracle.decode_one(t) ...; then tap.rows[i] is token i's
    result_norm (f32[n_embd]), tap.pre[i] the residual it was formed from, tap.plain[i] the norm
    without weight (and bias).  head: the output tensor (tied models: token_embd), recognised by
    the address of its data -- the oracles built from one GGUF image all read the same bytes."""

    def __init__(self, head):
        self.head = _addr(head.data)
        self.rows, self.pre, self.plain = [], [], []
        self._last = None

    def __enter__(self):
        self._mm, self._rms, self._ln = R.mul_mat_vec, R.rms_norm, R.layer_norm

        def mm(raw, t, K, x):
            if _addr(raw) == self.head:
                self.rows.append(np.array(x, np.float32))
                self.pre.append(self._last[0])
                self.plain.append(self._last[1])
            return self._mm(raw, t, K, x)

        def norm_of(f):
            def g(x, eps):
                y = f(x, eps)
                self._last = (np.array(x, np.float32), np.array(y, np.float32))
                return y
            return g

        R.mul_mat_vec, R.rms_norm, R.layer_norm = mm, norm_of(self._rms), norm_of(self._ln)
        return self

    def __exit__(self, *exc):
        R.mul_mat_vec, R.rms_norm, R.layer_norm = self._mm, self._rms, self._ln
        return False


def head_of(oracle):
    return oracle.tensors.get("output.weight", oracle.tensors["token_embd.weight"])


def oracle_rows(oracle, tokens):
    """(rows, pre, plain), each f32 [len(tokens)][n_embd]: the oracle decodes `tokens` one by one
    (continuing whatever its cache holds)."""
    with EmbdTap(head_of(oracle)) as tap:
        for t in tokens:
            oracle.decode_one(int(t))
    return np.stack(tap.rows), np.stack(tap.pre), np.stack(tap.plain)


def pool_mean(rows, n=None):
    """build_pooling MEAN: sum_t row_t * (1.0f / n), every term and every partial sum rounded to
    f32, in token order.  n: the divisor (default: the row count)."""
    rows = np.asarray(rows, np.float32)
    inv = np.float32(1.0) / np.float32(rows.shape[0] if n is None else n)
    acc = np.zeros(rows.shape[1], np.float32)
    for r in rows:
        acc = (acc + (r * inv).astype(np.float32)).astype(np.float32)
    return acc


def pool(rows, pooling):
    """The pooled row of llama_pooling_type `pooling` (1 MEAN, 2 CLS, 3 LAST)."""
    rows = np.asarray(rows, np.float32)
    return {1: pool_mean, 2: lambda r: r[0], 3: lambda r: r[-1]}[pooling](rows)


def embd_ulp_floor(buf, n_ctx, tokens, vec=None, runs=4, loras=None):
    """util.oracle_ulp_floor applied to the embedding rows: the oracle re-run `runs` times with every
    GEMV output (and attention score and head output) moved by -1, 0 or +1 ulp at random.  Returns
    all runs' rows, f32 [runs + 1][len(tokens)][n_embd], the unperturbed run first; floor_of() turns
    them into the per-output floor.  vec: the control vector of a steered oracle; loras: the
    [(lora_util.Adapter, scale)] of an adapted one."""
    tokens = [int(t) for t in tokens]
    with EmbdTap(head_of(util.oracle_from_gguf(buf, n_ctx=n_ctx))) as tap:
        if loras:
            import lora_util
            lora_util.lora_ulp_floor(buf, n_ctx, tokens[:1], tokens[1:], loras, vec, runs=runs)
        elif vec:
            cvec_util.cvec_ulp_floor(buf, n_ctx, tokens[:1], tokens[1:], vec, runs=runs)
        else:
            util.oracle_ulp_floor(buf, n_ctx, tokens[:1], tokens[1:], runs=runs)
    rows = np.stack(tap.rows)
    assert rows.shape[0] == (runs + 1) * len(tokens), rows.shape
    return rows.reshape(runs + 1, len(tokens), -1)


def floor_of(run_rows, reduce=None):
    """Per output: the largest max|perturbed - base| over the runs.  reduce: rows [n][n_embd] ->
    the outputs compared (default: the rows themselves; a pooled test passes its pooling)."""
    f = (lambda r: r) if reduce is None else reduce
    base = np.atleast_2d(f(run_rows[0])).astype(np.float64)
    floor = np.zeros(base.shape[0])
    for r in run_rows[1:]:
        floor = np.maximum(floor, np.max(np.abs(np.atleast_2d(f(r)).astype(np.float64) - base), axis=-1))
    return floor
