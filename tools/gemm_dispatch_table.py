"""The GEMM dispatcher's decisions over a sweep of shapes, layouts, dtypes, batches, workspace offers and A/B knobs, read from the two plan
queries of the C ABI (db1_gemm_kernel_choice, db1_gemm_workspace_bytes).  Both are host code: no GPU is needed.

    python tools/gemm_dispatch_table.py OUT.json      write the table
    python tools/gemm_dispatch_table.py               print a summary of the branch cases on default knobs

tests/golden/gemm_dispatch.json is this table as recorded at the commit BEFORE the dispatcher was restructured around one plan
(tests/test_host_cpu.py demands equality on every row): a change of a dispatch rule shows there as a diff of named rows.

Row = (shape, layout, dtC, batch0 x batch1, knob setting) -> the workspace need and six kernel-choice codes, one per (beta, offered
workspace) in the order of BETAS x OFFERS; a code is one character of CODE_CHARS (index = the code of db1_gemm_kernel_choice:
kernel | 16 split-K | 32 tail call)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32, BF16 = 0, 1
LAYOUTS = ("nt", "nn", "tn")
DTC = (("f32", F32), ("bf16", BF16))
BETAS = (0.0, 1.0)
OFFERS = ("any", "none", "need")            # offered workspace: -1 (whatever the plan needs) / 0 / exactly the queried need
BATCHES = ((1, 1), (16, 1), (4, 16))
KNOBS = (("default", None),) + tuple((f"{k}={v}", (k, v)) for k, vals in (
    ("w4", (0, 2)), ("w4n", (0, 1, 2, 5)), ("gemm_splitk", (0,)), ("gemm_halfwave", (1 << 20,)), ("tri_split", (0, 2)),
    ("gemm_tile", (128, 256, 512, 1024))) for v in vals)
CODE_CHARS = "0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ+/"
KERNELS = {0: "strided-fp32", 1: "tile128", 2: "tile256", 3: "pp-k64", 4: "pp-k32", 5: "w4", 6: "skinny", 7: "w4n"}


def step_shapes(T, d=2048):
    """the dense products of a layer + the head at T tokens, as tools/bench_kernels.py gemm times them: y = x W^T, dx = dy W, dW = dy^T x"""
    out = []
    for N, K in ((3 * d, d), (d, d), (4 * d, d), (d, 2 * d), (33280, d)):
        out += [(T, N, K), (T, K, N), (N, K, T)]
    return out


# one shape per branch of gemm_plan: (M, N, K), layout, dtC, beta, knob, offered workspace -> (kernel, split-K, tail call) on a single product
BRANCH_CASES = [
    ((16, 2048, 2048), "nt", "bf16", 0.0, None, "any", ("skinny", False, False)),
    ((256, 384, 192), "nt", "bf16", 0.0, None, "any", ("tile128", False, False)),
    ((256, 384, 192), "nn", "bf16", 0.0, None, "any", ("tile256", False, False)),
    ((64, 576, 8192), "tn", "f32", 1.0, None, "any", ("tile128", False, False)),
    ((512, 768, 320), "nn", "bf16", 0.0, None, "any", ("tile256", False, False)),
    ((2048, 128, 4096), "nn", "bf16", 0.0, None, "any", ("w4n", True, False)),
    ((2048, 128, 4096), "nn", "bf16", 0.0, ("w4n", 0), "any", ("tile256", True, False)),
    ((1024, 2048, 8192), "nt", "bf16", 0.0, None, "any", ("w4", True, False)),
    ((1024, 2048, 8192), "nn", "bf16", 0.0, None, "any", ("w4", True, False)),
    ((1024, 2048, 8192), "tn", "bf16", 0.0, None, "any", ("w4", True, False)),
    ((1024, 2048, 8192), "nn", "bf16", 0.0, ("w4", 0), "any", ("pp-k32", True, False)),
    ((1024, 2048, 8192), "nt", "bf16", 0.0, None, "none", ("tile128", False, False)),
    ((1024, 2048, 8192), "tn", "bf16", 0.0, None, "none", ("tile256", False, False)),
    ((4096, 2048, 2048), "nt", "bf16", 0.0, None, "any", ("w4n", False, False)),
    ((4096, 2048, 32768), "tn", "bf16", 0.0, None, "any", ("w4", True, False)),
    ((3072, 4096, 32768), "nn", "bf16", 0.0, None, "any", ("w4", True, False)),
    ((3072, 4096, 32768), "tn", "bf16", 0.0, None, "any", ("w4", True, False)),
    ((3072, 4096, 32768), "nt", "bf16", 0.0, None, "any", ("w4", False, False)),
    ((8448, 2048, 16384), "nt", "bf16", 0.0, None, "any", ("w4", False, True)),
    ((65536, 8192, 2048), "nt", "bf16", 0.0, None, "any", ("w4", False, False)),
    ((65536, 8192, 2048), "nt", "bf16", 0.0, ("w4", 0), "any", ("pp-k64", False, False)),
]


def sweep_shapes():
    seen, out = set(), []
    for s in step_shapes(4 * 1024) + step_shapes(64 * 1024) + [c[0] for c in BRANCH_CASES]:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


def strides(layout, M, N, K):
    """(a_rs, a_cs, b_rs, b_cs, c_rs, c_cs) of contiguous operands: nt = x [M, K], W [N, K]; nn = dy [M, K], W [K, N]; tn = dy [K, M], x [K, N]"""
    a = (K, 1) if layout != "tn" else (1, M)
    b = (1, K) if layout == "nt" else (N, 1)
    return a + b + (N, 1)


def query(lib, shape, layout, dtc, batch, beta, offer):
    """(code, workspace need) of one product"""
    M, N, K = shape
    st = strides(layout, M, N, K)
    need = int(lib.db1_gemm_workspace_bytes(M, N, K, BF16, BF16, dtc, *st, batch[0], batch[1]))
    ws = {"any": -1, "none": 0, "need": need}[offer]
    return int(lib.db1_gemm_kernel_choice(M, N, K, BF16, BF16, dtc, *st, batch[0], batch[1], float(beta), ws)), need


def with_knob(lib, knob, fn):
    lib.db1_test_clear_knobs()
    try:
        if knob is not None:
            assert lib.db1_test_set_knob(knob[0].encode(), int(knob[1])) == 0, knob
        return fn()
    finally:
        lib.db1_test_clear_knobs()


def table(lib=None):
    """{"M,N,K layout dtC b0xb1": {"ws": [need per knob], "codes": "6 characters per knob"}}"""
    if lib is None:
        from bdm_db1_amd import lib as db1lib
        lib = db1lib.load()
    rows = {}
    for shape in sweep_shapes():
        for layout in LAYOUTS:
            for dname, dtc in DTC:
                for batch in BATCHES:
                    ws, codes = [], ""
                    for _, knob in KNOBS:
                        def one():
                            got = [query(lib, shape, layout, dtc, batch, beta, offer) for beta in BETAS for offer in OFFERS]
                            return got[0][1], "".join(CODE_CHARS[c] for c, _ in got)
                        n, s = with_knob(lib, knob, one)
                        ws.append(n)
                        codes += s
                    rows["%d,%d,%d %s %s %dx%d" % (shape + (layout, dname) + batch)] = {"ws": ws, "codes": codes}
    return rows


def document(rows, header):
    return {"header": header, "knobs": [k for k, _ in KNOBS], "betas": list(BETAS), "offers": list(OFFERS), "code_chars": CODE_CHARS, "rows": rows}


def branch_choice(lib, case):
    shape, layout, dname, beta, knob, offer, _ = case
    code, need = with_knob(lib, knob, lambda: query(lib, shape, layout, dict(DTC)[dname], (1, 1), beta, offer))
    return (KERNELS[code & 15], bool(code & 16), bool(code & 32)), need


if __name__ == "__main__":
    from bdm_db1_amd import lib as db1lib
    L = db1lib.load()
    if len(sys.argv) > 1:
        doc = document(table(L), "GEMM dispatch table of bdm_db1_amd, recorded by tools/gemm_dispatch_table.py from THIS project's own library at the "
                                 "commit before the dispatcher was restructured around one plan (not from the reference project)")
        with open(sys.argv[1], "w") as f:
            json.dump(doc, f, separators=(",", ":"))
            f.write("\n")
        print(f"{len(doc['rows'])} rows x {len(KNOBS)} knob settings x {len(BETAS) * len(OFFERS)} queries -> {sys.argv[1]} ({os.path.getsize(sys.argv[1])} bytes)")
    else:
        for case in BRANCH_CASES:
            got, need = branch_choice(L, case)
            print(case[:6], "->", got, f"{need} B", "" if got == case[6] else f"  EXPECTED {case[6]}")
