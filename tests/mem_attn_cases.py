"""The (q, mlen, shift, nd) cases of db1_relattn_mem_fwd, shared by the CPU proof of the probe's margin (test_mem_attn_probe_cpu.py) and the
device test (test_mem_attn_kernels_gpu.py).  A workgroup owns 64 queries, a wave 16 of them, a step 32 keys:
  * a second and a third 64-query block, one of them holding a single row (65, 129, 130) and ragged last 16-row tiles (80, 100, 81, 70);
  * shift 0 -- what ``_window`` gives under same_length with a full memory, each query sees exactly mlen keys -- and 1, and old edges on,
    before and after a 32-key step (32, 33, 31 + 1 via 97 / 65);
  * mlen on, before and after a step (31, 32, 33) and a 128-key boundary (127, 128, 129);
  * nd < klen (only masked pairs reach the clamp), the caption prompt's 200 queries with distances past 256, one query, one-key windows."""

MEM_CASES = [
    (65, 0, 65, None), (80, 40, 120, None), (100, 129, 32, None), (129, 31, 160, None), (130, 127, 1, 140),
    (96, 300, 97, None), (200, 300, 500, None), (64, 128, 192, None), (127, 1, 128, None), (128, 32, 33, None),
    (192, 64, 256, None), (81, 128, 16, None), (160, 0, 17, None), (100, 64, 0, None), (65, 33, 0, None),
    (1, 40, 0, None), (130, 129, 0, None), (64, 1, 0, None), (70, 96, 0, 120),
]
ONE_KEY_CASE = (64, 1, 0, None)      # every row sees key i + 1 alone: out is blind to its distance, lse is not
