// kws_fast_maxmin.h -- the fast kernel's maxima, minima and activation clamps behind the FFT (kws_fast.hip), as single instructions.
// Device code only; tests/fast_maxmin/ compiles this header into a stand-alone program and holds every helper against fmaxf / fminf on the device.
#pragma once

// fast_max / fast_min: fmaxf / fminf as exactly ONE v_max_f32 / v_min_f32.  The compiler's own fmaxf is the same instruction behind a canonicalising
// v_max_f32 x, x, x for every operand it cannot prove is no signalling NaN -- an accumulator of a matrix instruction, a value read back from LDS, the result
// of a select -- because in IEEE mode the instruction would quiet one and fmaxf must not (profiles/net_lean.md: half of the network half's v_max_f32).
// Signalling NaNs are left out of these helpers' contract: no arithmetic of this kernel produces one (every NaN an instruction creates is quiet), so the
// canonicalisation never changed a bit.  Everything else is the instruction's own behaviour, which is what fmaxf / fminf compiled to all along: a quiet NaN
// operand is dropped (both NaN: NaN), zeros of either sign are ordered as the instruction orders them, infinities and subnormals are ordinary values (the kernel runs with fp32 denormals on).
// tests/fast_maxmin/ holds the pair against fmaxf / fminf on the device.  Not volatile: dead results go, the scheduler moves them like any other
// instruction -- but the compiler does not SPECULATE an asm, so a maximum that used to sit in one arm of a select is taken unconditionally in front of it.
// _u: the second operand MUST be wave-uniform -- an activation bound read from the plan (KwsFastBlock::*_min / *_max, KwsFastPlan::fc_*) -- and stays in its
// scalar register.  This is a requirement on the caller, not a hint: for a bound that differs between lanes the "s" constraint makes the compiler read lane
// 0's value for every lane, without a diagnostic.  A per-lane bound takes fast_max / fast_min.
__device__ __forceinline__ float fast_max(float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float fast_min(float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ float fast_max_u(float a, float b) { float r; asm("v_max_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(b)); return r; }
__device__ __forceinline__ float fast_min_u(float a, float b) { float r; asm("v_min_f32 %0, %2, %1" : "=v"(r) : "v"(a), "s"(b)); return r; }
// max(|a|, |b|): the absolute values as the instruction's source modifiers
__device__ __forceinline__ float fast_max_abs(float a, float b) { float r; asm("v_max_f32 %0, |%1|, |%2|" : "=v"(r) : "v"(a), "v"(b)); return r; }
// fminf(fmaxf(v, lo), hi) with wave-uniform bounds
__device__ __forceinline__ float fast_clamp_u(float v, float lo, float hi) { return fast_min_u(fast_max_u(v, lo), hi); }
