"""Diagnostic: time layer 0's segment sums (kl_test_segment_sums) at the flagship window's shape, kernel by kernel.

  python3 tools/probe_segsum.py [streams] [context values in the batch]

Ids as bench.py draws them: characters from its synthetic corpus' Zipf-like distribution, one context value per stream."""
import sys
import numpy as np
import torch
sys.path.insert(0, '.')
from ocrd_keraslm_amd.lib import hipabi
lib = hipabi.load()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 3072
n_values = int(sys.argv[2]) if len(sys.argv) > 2 else 200
T, cols, V, R = 256, 2048, 256, 200
rng = np.random.default_rng(7)
p = 1.0 / np.arange(1, V + 1)
idx = torch.from_numpy(rng.choice(V, size=(B, T), p=p / p.sum()).astype(np.int32)).cuda()
ctx = torch.from_numpy(rng.integers(0, n_values, size=(B, 1, 1)).repeat(T, axis=1).astype(np.int32)).cuda()
dZ = (torch.rand((B * T, cols), device='cuda') - 0.5).to(torch.bfloat16)
dEK = torch.empty((V, cols), device='cuda')
dCtxK = torch.empty((R, cols), device='cuda')
ws = torch.empty(lib.kl_test_segment_sums_ws_bytes(B, T, 1, V, R), dtype=torch.uint8, device='cuda')
s = torch.cuda.current_stream().cuda_stream


def run():
    rc = lib.kl_test_segment_sums(dZ.data_ptr(), cols, B, T, cols, idx.data_ptr(), ctx.data_ptr(), 1, V, R, dEK.data_ptr(),
                                  dCtxK.data_ptr(), ws.data_ptr(), s)
    assert rc == 0, rc


run(); torch.cuda.synchronize()
pairs = len(np.unique(idx.cpu().numpy().astype(np.int64) * R + ctx[:, :, 0].cpu().numpy()))
ref = torch.zeros((R, cols), device='cuda').index_add_(0, ctx[:, :, 0].T.reshape(-1).long(), dZ.float())
err = ((dCtxK - ref).abs().max() / ref.abs().max()).item()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
n = 10
e0.record()
for _ in range(n):
    run()
e1.record(); torch.cuda.synchronize()
ms = e0.elapsed_time(e1) / n
print(f"B={B} T={T} cols={cols} pairs={pairs}: {ms * 1e3:8.1f} us per call, {B * T * cols * 2 / ms / 1e9:6.2f} TB/s over dZ; "
      f"context sums off by {err:.2e} of their max")
