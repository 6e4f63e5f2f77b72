// The K pipeline of the fp32-MFMA implicit-GEMM kernels (conv_igemm.hip, conv_bn_kernel.h), included INSIDE the kernel
// body: as a function template over the callables the same statements compile to other code (profiles/
// conv_split_machine_code.md), as text they compile to the parent's.  The including kernel provides
//   DEPTH                 1 | 2 register sets (compile-time), nsteps, the load cursor (tap, c)
//   advance()             the cursor one K step on
//   load_set(Set, tap, c) request the cursor's operand tiles into register set Set
//   store_set(Set, buf)   write that set to LDS buffer buf
//   load_step(tap, c), store_step(buf)   the same with set 0, as lambdas of the kernel's own: what DEPTH = 1 calls (calling
//                         load_set / store_set directly there compiles to other code as well)
//   mfma_step(buf)        the step's MFMAs out of LDS buffer buf
// and may define the statement macros CONV_MFMA_AFTER_REQUESTS / CONV_MFMA_AFTER_FIRST_TILE ("prologue requests issued" /
// "first tile in LDS and visible"): a profiling build's time stamps (conv_bn_kernel.h).
// DEPTH = 1: the loads of K step t + 1 are issued before the MFMAs of step t and stored to the other buffer after them.
// DEPTH = 2 (round 6; BT = 64, one wave group): the operand tiles of a K step are requested two steps ahead into two
// register sets -- a 64 x 64 tile's K step is 16 MFMAs per wave (0.43 us), less than a global round trip under load, so
// with one step of cover every step ended in a wait for its successor's tiles.
if constexpr (DEPTH == 1) {
  load_step(tap, c);
  store_step(0);
  __syncthreads();
  for (int step = 0; step < nsteps; step++) {
    const int buf = step & 1;
    const bool more = step + 1 < nsteps;
    if (more) {
      advance();
      load_step(tap, c);            // in flight during the MFMAs below
    }
    mfma_step(buf);
    if (more) store_step(buf ^ 1);   // the other buffer: its last readers passed the barrier of the previous step
    __syncthreads();
  }
} else {
  // At the top of turn s: LDS buffer (s & 1) holds step s; register set (s + 1) & 1 holds step s + 1 (in flight); set
  // (s & 1) is free and takes step s + 2.  The steady-state turns request unconditionally, so that hipcc's wait before
  // the LDS stores of step s + 1 leaves the just-issued loads of step s + 2 in flight (vmcnt(7) / (5) / (4) in the ISA;
  // a conditional request makes it wait for everything).  conv_bn's <64, 32, 1>: 124 VGPRs, no scratch (a generic
  // DEPTH-turn formulation with a switch over the last turns spilled: 128 VGPRs + 76 B of scratch at depth 2, 208 B at
  // depth 3).
  // Round 6, measured and not kept: a scheduling fence behind the requests (hipcc sinks the four buffer loads below
  // twelve of the step's sixteen MFMAs; with the fence it serialises the LDS reads instead: + 2 % per layer) and
  // s_setprio 1 around the MFMAs (+ 2 %): profiles/r06_conv_prefetch.md.
  static_assert(DEPTH == 2, "two register sets");
  load_set(Set0{}, tap, c);
  if (nsteps > 1) {
    advance();
    load_set(Set1{}, tap, c);
  }
#ifdef CONV_MFMA_AFTER_REQUESTS
  CONV_MFMA_AFTER_REQUESTS
#endif
  store_set(Set0{}, 0);
  __syncthreads();
#ifdef CONV_MFMA_AFTER_FIRST_TILE
  CONV_MFMA_AFTER_FIRST_TILE
#endif
  int step = 0;
  for (; step + 3 < nsteps; step += 2) {
    advance();
    load_set(Set0{}, tap, c);        // step + 2
    mfma_step(0);
    store_set(Set1{}, 1);            // step + 1
    __syncthreads();
    advance();
    load_set(Set1{}, tap, c);        // step + 3
    mfma_step(1);
    store_set(Set0{}, 0);            // step + 2
    __syncthreads();
  }
  while (step < nsteps) {            // the last one to three steps
    if (step + 2 < nsteps) {
      advance();
      load_set(Set0{}, tap, c);
    }
    mfma_step(0);
    if (step + 1 < nsteps) store_set(Set1{}, 1);
    __syncthreads();
    if (++step >= nsteps) break;
    if (step + 2 < nsteps) {
      advance();
      load_set(Set1{}, tap, c);
    }
    mfma_step(1);
    if (step + 1 < nsteps) store_set(Set0{}, 0);
    __syncthreads();
    ++step;
  }
}
