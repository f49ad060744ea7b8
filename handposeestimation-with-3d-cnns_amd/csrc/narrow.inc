// narrow.inc — the store side of a kernel that writes float16 / bfloat16 volumes: tsdf_lowp.hip and tsdf_maplowp.hip
// include it (inside their anonymous namespace, after <hip/hip_runtime.h> and include/tsdf_lowp.h); the product does not.
//   narrow2      two float32 -> one 32-bit word of two 2-byte values, round-to-nearest-even
//   store_vol    one 16-byte or 8-byte store of the output volume with the scope bits of TSDF_LOWP_STORE_ASM
//   Piece<V>     the vector type a lane's V voxels of one channel leave in
//   bad_dtype    host: the dtype test of an entry
// No device globals.  All stores are vector stores.

typedef float lowp_f2 __attribute__((ext_vector_type(2)));
typedef unsigned lowp_u4 __attribute__((ext_vector_type(4)));
typedef unsigned lowp_u2 __attribute__((ext_vector_type(2)));
typedef _Float16 lowp_h2 __attribute__((ext_vector_type(2)));
typedef __bf16 lowp_b2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) void *GlobalOut;

// Two float32 narrowed by round-to-nearest-even into one 32-bit word, the first in the low half.  float16: v_cvt_f16_f32
// (the kernels run with float16 subnormals on); bfloat16: v_cvt_pk_bf16_f32, gfx950's own conversion.
template <bool BF16>
__device__ __forceinline__ unsigned narrow2(float lo, float hi) {
  const lowp_f2 v = {lo, hi};
  if constexpr (BF16) {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, lowp_b2));
  } else {
    return __builtin_bit_cast(unsigned, __builtin_convertvector(v, lowp_h2));
  }
}

#ifndef TSDF_LOWP_STORE_ASM
#define TSDF_LOWP_STORE_ASM "nt"
#endif
// One store of the output volume: 16 bytes (8 voxels) or 8 bytes (4 voxels).  There is no builtin for the scope bits of
// a plain store, hence the inline assembly; the s_nop covers the "VALU overwrites the data registers of a wide store"
// hazard the compiler can no longer see (as in the product's store_vol4).
__device__ __forceinline__ void store_vol(GlobalOut p, lowp_u4 v) {
  asm volatile("global_store_dwordx4 %0, %1, off " TSDF_LOWP_STORE_ASM "\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ void store_vol(GlobalOut p, lowp_u2 v) {
  asm volatile("global_store_dwordx2 %0, %1, off " TSDF_LOWP_STORE_ASM "\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}

template <int V>
struct Piece;
template <>
struct Piece<8> {
  typedef lowp_u4 type;
};
template <>
struct Piece<4> {
  typedef lowp_u2 type;
};

bool bad_dtype(int dtype) { return dtype != TSDF_LOWP_F16 && dtype != TSDF_LOWP_BF16; }
