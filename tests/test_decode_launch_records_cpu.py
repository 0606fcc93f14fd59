"""The seven capturable decoding wrappers of ops.py, launch by launch, without a GPU: every wrapper is called on small CPU tensors with
``ops.P``, ``ops.stream`` and ``lib.call`` replaced by recorders, and the C symbol, the whole argument list (order, values, NULLs) or the
exception text must equal the records in test_decode_launch_records_cpu.json.  The records were written by this file's own helper
(``python tests/test_decode_launch_records_cpu.py --write``) on the commit BEFORE the wrappers' checks were moved into shared helpers; the
helper calls only the public wrappers, so it runs on both sides of that change.  V = 5 in a row stride of 8, M = 2 logits rows, S = 3 slots,
max_new = 4, top_n = 2, capacities (2, 1): the smallest case where ld != V, S != M and every optional buffer exists."""
import contextlib
import ctypes
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

torch = pytest.importorskip("torch")

FIXTURE = os.path.splitext(os.path.abspath(__file__))[0] + ".json"
V, LD, M, S, MX, TOP_N, BAD_CAP, BIAS_CAP = 5, 8, 2, 3, 4, 2, 2, 1
SEED = (7 << 32) | 0x9ABCDEF1                    # a 64-bit seed above 2^32: both halves reach the launch
F32, BF16, I32, I64 = torch.float32, torch.bfloat16, torch.int32, torch.int64


# ----------------------------------------------------------------------------------------------------------------------------- recording
@contextlib.contextmanager
def _recording(names, calls):
    """``ops.P`` -> the tensor's name in ``names`` (by id; None: "NULL"), ``ops.stream`` -> "STREAM", ``lib.call`` -> appended to ``calls``"""
    from bdm_db1_amd import lib, ops

    def render(symbol, a):
        if isinstance(a, ctypes.c_void_p):
            return "NULL" if not a.value else hex(a.value)
        if isinstance(a, (str, float)):
            return a
        assert isinstance(a, (int, np.integer)), (symbol, a)
        return int(a)

    def call(symbol, *args):
        calls.append([symbol, [render(symbol, a) for a in args]])

    saved = ops.P, ops.stream, lib.call
    ops.P = lambda t: "NULL" if t is None else names.get(id(t), "?")
    ops.stream = lambda: "STREAM"
    lib.call = call
    try:
        yield
    finally:
        ops.P, ops.stream, lib.call = saved


def _tensors(slots, dtype):
    z = lambda *shape, dt=I32: torch.zeros(*shape, dtype=dt)
    return dict(logits=torch.zeros(M, LD, dtype=dtype)[:, :V], t1=z(1), t=z(slots), limit=z(slots), finished=z(slots), lengths=z(slots),
                status=z(slots), stream_id=z(slots), checked=z(slots), stop_hit=z(slots), out=z(slots, MX),
                next_ids=z(slots, 2, dt=I64)[:, 0], row_map=z(M), logprob=z(slots, MX, dt=F32), sum_logprob=z(slots, dt=F32),
                top_ids=z(slots, MX, TOP_N), top_logprob=z(slots, MX, TOP_N, dt=F32), params=z(slots, 8), cons=z(slots, 8),
                bad1=z(BAD_CAP), bias_ids1=z(BIAS_CAP), bias_val1=z(BIAS_CAP, dt=F32), bad=z(slots, BAD_CAP), bias_ids=z(slots, BIAS_CAP),
                bias_val=z(slots, BIAS_CAP, dt=F32), stop_tok=z(2, 16), stop_len=z(2), stop_tok_per=z(slots, 16, 16), stop_len_per=z(slots, 16))


def _callers():
    from bdm_db1_amd import ops
    g = lambda T, *names: [T[n] for n in names]
    state = ("finished", "lengths", "out", "next_ids", "status")
    stop = ("lengths", "checked", "finished", "stop_hit", "out", "next_ids")
    return {
        "select_tokens": lambda T, kw: ops.select_tokens(*g(T, "logits", "t1", *state), **kw),
        "select_tokens_slots": lambda T, kw: ops.select_tokens_slots(*g(T, "logits", "t", "limit", *state), **kw),
        "select_tokens_slots_per": lambda T, kw: ops.select_tokens_slots_per(*g(T, "logits", "params", "t", "limit", *state), **kw),
        "constrain_logits": lambda T, kw: ops.constrain_logits(*g(T, "logits", "t", "out"), **kw),
        "constrain_logits_slots_per": lambda T, kw: ops.constrain_logits_slots_per(*g(T, "logits", "cons", "t", "out", "finished", "status"), **kw),
        "stop_match": lambda T, kw: ops.stop_match(*g(T, "stop_tok", "stop_len", *stop), **kw),
        "stop_match_per": lambda T, kw: ops.stop_match_per(*g(T, "stop_tok_per", "stop_len_per", *stop), **kw),
    }


def record(wrapper, slots, dtype, kw, fault=None):
    """one call of ``wrapper`` over fresh tensors of ``slots`` slots; a keyword value "@name" is the tensor of that name; ``fault(T, kw)``
    breaks one thing first -> {"calls": [[symbol, [args]]], "error": None or "Type: text"}"""
    T, kw = _tensors(slots, dtype), dict(kw)
    if fault is not None:
        fault(T, kw)
    kw = {k: T[v[1:]] if isinstance(v, str) and v.startswith("@") else v for k, v in kw.items()}
    names, calls, error = {id(v): k for k, v in T.items() if torch.is_tensor(v)}, [], None
    with _recording(names, calls):
        try:
            _callers()[wrapper](T, kw)
        except Exception as e:  # noqa: BLE001  (whatever it raises today is the record)
            error = f"{type(e).__name__}: {e}"
    return dict(calls=calls, error=error)


# --------------------------------------------------------------------------------------------------------------------------------- cases
LP = dict(logprob="@logprob", sum_logprob="@sum_logprob")
TOP = dict(LP, top_n=TOP_N, top_ids="@top_ids", top_logprob="@top_logprob")
MODES = dict(plain={}, lp=LP, top=TOP)
COMMON = dict(V=V, eos_id=4, pad_id=1, step_base=2, stream_id="@stream_id")
PICKS = dict(greedy=dict(vocab_lo=1, vocab_hi=4), sampled=dict(vocab_lo=1, vocab_hi=4, greedy=False, temperature=0.7, top_k=3, top_p=0.9, seed=SEED))
RM = dict(none=(M, {}), row_map=(S, dict(row_map="@row_map")))          # (slots, keywords): without a row_map row i is slot i and S = M
CON = dict(V=V, finished="@finished", repetition_penalty=1.3, no_repeat_ngram_size=2, bad="@bad1", eos_id=4, min_new=2)
CONS = dict(base=CON, freq=dict(CON, frequency_penalty=0.25), bias=dict(CON, bias_ids="@bias_ids1", bias_val="@bias_val1"))
TABLES = {"0_0": {}, "2_1": dict(bad="@bad", bias_ids="@bias_ids", bias_val="@bias_val")}


def _t_one(T, kw):
    T["t"] = T.pop("t1")


def _valid():
    for dn, dt in (("fp32", F32), ("bf16", BF16)):
        for mn, mode in MODES.items():
            for pn, pick in PICKS.items():
                yield f"select_tokens/{dn}/{mn}/{pn}", "select_tokens", M, dt, dict(COMMON, **pick, **mode), None
                for rn, (slots, rm) in RM.items():
                    yield f"select_tokens_slots/{dn}/{mn}/{pn}/{rn}", "select_tokens_slots", slots, dt, dict(COMMON, **pick, **mode, **rm), None
            for rn, (slots, rm) in RM.items():
                yield f"select_tokens_slots_per/{dn}/{mn}/{rn}", "select_tokens_slots_per", slots, dt, dict(COMMON, **mode, **rm), None
        for rn, (slots, rm) in RM.items():
            for cn, con in CONS.items():
                yield f"constrain_logits/{dn}/{cn}/t_1/{rn}", "constrain_logits", slots, dt, dict(con, **rm), _t_one
                yield f"constrain_logits/{dn}/{cn}/t_S/{rn}", "constrain_logits", slots, dt, dict(con, **rm), None
            for tn, tab in TABLES.items():
                yield (f"constrain_logits_slots_per/{dn}/{tn}/{rn}", "constrain_logits_slots_per", slots, dt, dict(V=V, eos_id=4, **tab, **rm), None)
        yield f"select_tokens/{dn}/defaults", "select_tokens", M, dt, {}, None
        yield f"select_tokens_slots/{dn}/defaults", "select_tokens_slots", M, dt, {}, None
        yield f"select_tokens_slots_per/{dn}/defaults", "select_tokens_slots_per", M, dt, {}, None
        yield f"constrain_logits/{dn}/defaults", "constrain_logits", M, dt, {}, None
        yield f"constrain_logits_slots_per/{dn}/defaults", "constrain_logits_slots_per", M, dt, {}, None
    for mn, mode in MODES.items():
        for rn, (slots, rm) in RM.items():
            yield f"stop_match/{mn}/{rn}", "stop_match", slots, F32, dict(pad_id=1, **mode, **rm), None
            yield f"stop_match_per/{mn}/{rn}", "stop_match_per", slots, F32, dict(pad_id=1, **mode, **rm), None


# ---- single faults: each breaks ONE thing in a call that is otherwise valid (S = 3 slots, a row_map, every optional buffer)
def put(name, make):
    return lambda T, kw: T.__setitem__(name, make(T[name]))


def arg(**new):
    return lambda T, kw: kw.update(new)


def drop(*names):
    return lambda T, kw: [kw.pop(n) for n in names]


longer = lambda x: torch.zeros(x.numel() + 1, dtype=x.dtype)                 # a vector with one element too many
wider = lambda x: torch.zeros(*x.shape[:-1], x.shape[-1] + 1, dtype=x.dtype)   # one column too many
as64 = lambda x: x.to(I64 if x.dtype == I32 else torch.float64)              # the wrong dtype
strided = lambda x: torch.zeros(x.numel() * 2, dtype=x.dtype)[::2]           # not contiguous
off_by_4 = lambda x: torch.zeros(x.numel() + 9, dtype=x.dtype)[1:1 + x.numel()].view(x.shape)   # contiguous, not 32-byte aligned
LOGITS = [("logits_3d", put("logits", lambda x: x[None])), ("logits_stride", put("logits", lambda x: torch.zeros(M, 2 * V)[:, ::2])),
          ("logits_f16", put("logits", lambda x: x.half())), ("V_0", arg(V=0)), ("V_6", arg(V=V + 1))]
WINDOW = [("window_empty", arg(vocab_lo=3, vocab_hi=3)), ("window_outside", arg(vocab_hi=V + 1)), ("window_negative", arg(vocab_lo=-1))]
SAMPLING = [("temperature_0", arg(temperature=0.0)), ("temperature_inf", arg(temperature=float("inf"))), ("top_p_0", arg(top_p=0.0)),
            ("top_p_above_1", arg(top_p=1.5)), ("top_k_negative", arg(top_k=-1))]
OUTPUTS = [("out_i64", put("out", as64)), ("out_1d", put("out", lambda x: x.reshape(-1))), ("out_rows", put("out", lambda x: torch.zeros(S + 1, MX, dtype=I32))),
           ("next_ids_i32", put("next_ids", lambda x: x.to(I32))), ("next_ids_rows", put("next_ids", longer)),
           ("next_ids_2d", put("next_ids", lambda x: torch.zeros(S, 2, dtype=I64))),
           ("logprob_alone", drop("sum_logprob")), ("sum_logprob_alone", drop("logprob")), ("logprob_wide", put("logprob", wider)),
           ("logprob_f64", put("logprob", as64)), ("sum_logprob_long", put("sum_logprob", longer)), ("top_n_alone", drop("top_ids", "top_logprob")),
           ("top_ids_missing", drop("top_ids")), ("top_logprob_missing", drop("top_logprob")), ("top_n_missing", drop("top_n")),
           ("top_n_0", arg(top_n=0)), ("top_n_17", arg(top_n=17)), ("top_n_bool", arg(top_n=True)), ("top_n_float", arg(top_n=2.0)),
           ("top_n_3", arg(top_n=3)), ("top_ids_i64", put("top_ids", as64)), ("top_logprob_wide", put("top_logprob", wider)),
           ("top_without_lp", drop("logprob", "sum_logprob"))]
ROW_MAP = [("row_map_long", put("row_map", longer)), ("row_map_i64", put("row_map", as64)), ("row_map_strided", put("row_map", strided))]


def vectors(*names):
    return [(f"{n}_long", put(n, longer)) for n in names] + [(f"{n}_i64", put(n, as64)) for n in names[:1]] + \
           [(f"{n}_strided", put(n, strided)) for n in names[:1]]


def _faults():
    sel = dict(COMMON, **PICKS["sampled"], **TOP)
    slot = ("t", "limit", "finished", "lengths", "status", "stream_id")
    for name, f in LOGITS + WINDOW + SAMPLING + vectors("finished", "lengths", "status", "t1", "stream_id") + OUTPUTS:
        yield f"select_tokens/fault/{name}", "select_tokens", M, F32, sel, f
    fewer_slots = [("fewer_slots_than_rows", lambda T, kw: T.update({k: T[k][:1].clone() for k in slot + ("out", "next_ids", "logprob", "sum_logprob",
                                                                                                        "top_ids", "top_logprob", "params", "cons")}))]
    for name, f in LOGITS + WINDOW + SAMPLING + ROW_MAP + fewer_slots + vectors(*slot) + OUTPUTS:
        yield f"select_tokens_slots/fault/{name}", "select_tokens_slots", S, F32, dict(sel, row_map="@row_map"), f
    params = [("params_none", put("params", lambda x: None)), ("params_wide", put("params", wider)), ("params_i64", put("params", as64)),
              ("params_rows", put("params", lambda x: torch.zeros(S + 1, 8, dtype=I32))), ("params_unaligned", put("params", off_by_4))]
    for name, f in LOGITS + ROW_MAP + fewer_slots + vectors(*slot) + params + OUTPUTS:
        yield f"select_tokens_slots_per/fault/{name}", "select_tokens_slots_per", S, F32, dict(COMMON, **TOP, row_map="@row_map"), f
    hist = [("hist_none", put("out", lambda x: None)), ("hist_1d", put("out", lambda x: x.reshape(-1))), ("hist_i64", put("out", as64)),
            ("hist_4097", put("out", lambda x: torch.zeros(S, 4097, dtype=I32))), ("hist_0", put("out", lambda x: torch.zeros(S, 0, dtype=I32))),
            ("hist_strided", put("out", lambda x: torch.zeros(S, 2 * MX, dtype=I32)[:, ::2])),
            ("hist_fewer_slots_than_rows", put("out", lambda x: x[:1].clone())),
            ("hist_rows_without_row_map", drop("row_map"))]
    con = [("t_list", put("t", lambda x: [0, 0, 0])), ("bad_list", arg(bad=[1, 2])), ("bad_1025", arg(bad=torch.zeros(1025, dtype=I32))),
           ("bad_i64", put("bad1", as64)), ("bad_strided", put("bad1", strided)), ("t_2_of_3", put("t", lambda x: x[:2].clone())),
           ("t_i64", put("t", as64)), ("finished_long", put("finished", longer)), ("finished_i64", put("finished", as64)),
           ("theta_0", arg(repetition_penalty=0.0)), ("theta_negative", arg(repetition_penalty=-1.0)), ("theta_inf", arg(repetition_penalty=float("inf"))),
           ("theta_nan", arg(repetition_penalty=float("nan"))), ("theta_1e-39", arg(repetition_penalty=1e-39)), ("theta_1e39", arg(repetition_penalty=1e39)),
           ("ngram_negative", arg(no_repeat_ngram_size=-1)), ("min_new_negative", arg(min_new=-1)), ("freq_inf", arg(frequency_penalty=float("inf"))),
           ("pres_nan", arg(presence_penalty=float("nan"))), ("freq_1e39", arg(frequency_penalty=1e39)), ("bias_ids_alone", drop("bias_val")),
           ("bias_val_alone", drop("bias_ids")), ("bias_ids_list", arg(bias_ids=[1])), ("bias_lengths", put("bias_val1", longer)),
           ("bias_1025", arg(bias_ids=torch.zeros(1025, dtype=I32), bias_val=torch.zeros(1025, dtype=F32))), ("bias_ids_i64", put("bias_ids1", as64)),
           ("bias_val_f64", put("bias_val1", as64))]
    full = dict(CONS["bias"], frequency_penalty=0.25, presence_penalty=-0.5, row_map="@row_map")
    for name, f in hist + LOGITS + ROW_MAP + con:
        yield f"constrain_logits/fault/{name}", "constrain_logits", S, F32, full, f
    tables = [("bad_1d", put("bad", lambda x: x.reshape(-1))), ("bias_ids_1d", put("bias_ids", lambda x: x.reshape(-1))), ("bias_val_list", arg(bias_val=[[0.0]] * S)),
              ("bias_widths", put("bias_val", wider)), ("bias_ids_alone", drop("bias_val")), ("bad_1025", put("bad", lambda x: torch.zeros(S, 1025, dtype=I32))),
              ("bias_1025", lambda T, kw: T.update(bias_ids=torch.zeros(S, 1025, dtype=I32), bias_val=torch.zeros(S, 1025, dtype=F32))),
              ("t_none", put("t", lambda x: None)), ("finished_none", put("finished", lambda x: None)), ("status_none", put("status", lambda x: None)),
              ("cons_none", put("cons", lambda x: None)), ("cons_wide", put("cons", wider)), ("cons_i64", put("cons", as64)),
              ("cons_unaligned", put("cons", off_by_4)), ("bad_i64", put("bad", as64)), ("bad_rows", put("bad", lambda x: torch.zeros(S + 1, BAD_CAP, dtype=I32))),
              ("bias_ids_i64", put("bias_ids", as64)), ("bias_val_f64", put("bias_val", as64))]
    for name, f in hist + LOGITS + ROW_MAP + vectors("t", "finished", "status") + tables:
        yield (f"constrain_logits_slots_per/fault/{name}", "constrain_logits_slots_per", S, F32,
               dict(V=V, eos_id=4, **TABLES["2_1"], row_map="@row_map"), f)
    out = [("out_none", put("out", lambda x: None)), ("out_1d", put("out", lambda x: x.reshape(-1))), ("out_i64", put("out", as64)),
           ("out_0", put("out", lambda x: torch.zeros(S, 0, dtype=I32)))]
    rows = [("row_map_more_rows_than_slots", put("row_map", lambda x: torch.zeros(S + 1, dtype=I32))), ("row_map_empty", put("row_map", lambda x: x[:0].clone())),
            ("row_map_i64", put("row_map", as64)), ("row_map_strided", put("row_map", strided))]
    state = vectors("lengths", "checked", "finished", "stop_hit")
    outputs = [(n, f) for n, f in OUTPUTS if not n.startswith("out_")]
    lists = [("stop_tok_none", put("stop_tok", lambda x: None)), ("stop_len_list", put("stop_len", lambda x: [1, 1])), ("stop_tok_1d", put("stop_tok", lambda x: x.reshape(-1))),
             ("stop_tok_0", put("stop_tok", lambda x: x[:0].clone())), ("stop_tok_17", put("stop_tok", lambda x: torch.zeros(17, 16, dtype=I32))),
             ("stop_tok_15_wide", put("stop_tok", lambda x: torch.zeros(2, 15, dtype=I32))), ("stop_tok_i64", put("stop_tok", as64)),
             ("stop_len_long", put("stop_len", longer)), ("stop_len_i64", put("stop_len", as64))]
    for name, f in out + lists + state + rows + outputs:
        yield f"stop_match/fault/{name}", "stop_match", S, F32, dict(pad_id=1, **TOP, row_map="@row_map"), f
    per = [("stop_tok_none", put("stop_tok_per", lambda x: None)), ("stop_len_list", put("stop_len_per", lambda x: [[1] * 16] * S)),
           ("stop_tok_2d", put("stop_tok_per", lambda x: x[0].clone())), ("stop_tok_rows", put("stop_tok_per", lambda x: torch.zeros(S + 1, 16, 16, dtype=I32))),
           ("stop_tok_i64", put("stop_tok_per", as64)), ("stop_len_wide", put("stop_len_per", wider)), ("stop_len_i64", put("stop_len_per", as64))]
    for name, f in out + per + state + rows + outputs:
        yield f"stop_match_per/fault/{name}", "stop_match_per", S, F32, dict(pad_id=1, **TOP, row_map="@row_map"), f


def all_records():
    got = {}
    for name, wrapper, slots, dtype, kw, fault in list(_valid()) + list(_faults()):
        assert name not in got, name
        got[name] = record(wrapper, slots, dtype, kw, fault)
    return got


# --------------------------------------------------------------------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def records():
    from bdm_db1_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libdb1_hip.so is not built")        # (the wrappers ask the library's own *_supported predicates)
    with open(FIXTURE) as f:
        return all_records(), json.load(f)


def test_every_launch_and_every_refusal_is_what_it_was(records):
    got, want = records
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_the_cases_cover_what_they_claim(records):
    """every valid case launched exactly once, every fault raised without a launch, and every entry point of the seven wrappers is reached"""
    got, _ = records
    for name, r in got.items():
        if "/fault/" in name:
            assert r["error"] is not None and r["calls"] == [], (name, r)
        else:
            assert r["error"] is None and len(r["calls"]) == 1, (name, r)
    symbols = {r["calls"][0][0] for r in got.values() if r["calls"]}
    assert symbols == {"db1_select_tokens", "db1_select_tokens_lp", "db1_select_tokens_top", "db1_select_tokens_slots", "db1_select_tokens_slots_lp",
                       "db1_select_tokens_slots_top", "db1_select_tokens_slots_per", "db1_constrain_logits", "db1_constrain_logits_pen",
                       "db1_constrain_logits_slots_per", "db1_stop_match", "db1_stop_match_per"}
    # the recorder named every pointer: nothing unnamed reached a launch, and the seed arrived in two halves
    assert not any("?" in map(str, r["calls"][0][1]) for r in got.values() if r["calls"])
    args = got["select_tokens/fp32/plain/sampled"]["calls"][0][1]
    assert SEED & 0xFFFFFFFF in args and SEED >> 32 in args and args[0] == "logits" and args[-1] == "STREAM" and args[3] == LD


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit("usage: python tests/test_decode_launch_records_cpu.py --write   (run it on the commit whose launches are to be pinned)")
    with open(FIXTURE, "w") as f:
        json.dump(all_records(), f, indent=0, sort_keys=True)
        f.write("\n")
