"""The measured fp32 terms of the op-level decode tests (tests/test_gpu_decode_ops.py).  Each is 8 x the largest
|fp32 numpy restatement - fp64 reference| over the planted inputs of tests/chat_ref.py (8: another summation order and the
hardware exp2 / exp); tests/test_cpu_chat_ref.py re-derives each and asserts the constant is not smaller."""
ATTN_FP32_TERM = 1.5e-5      # decode attention: re-derived 1.44e-5 (worst case spike_first_prompt, |out| up to 4)
ACCUM_FP32_TERM = 7e-6       # x + alpha * sum of the planes: re-derived 6.72e-6 (17 planes, |x| up to ~10); MI355X: worst 7.4e-7
SWIGLU_FP32_TERM = 1.4e-5    # silu(gate) * up of fp32 GEMM rows: re-derived 1.38e-5
