// device.inc — the host preamble of every library here: every tsdf_*.hip here, the product's and each extension's,
// includes it, so "is this a device the code object runs on", the two return idioms of an entry point and the resolution
// rule exist once.  Host code only; it exports nothing.
// (The device primitives that exist once are in prim.inc.)
//   check_device   the current device is a gfx950
//   device_cus     its CU count, for an entry that sizes a grid by it
//   launched       the status an entry returns after its launch
//   misaligned     the alignment test of a pointer argument
//   bad_res        the resolution rule of an extension's entry
//
// Included inside an anonymous namespace, after <hip/hip_runtime.h>, <stdint.h>, <string.h>, <atomic> and include/tsdf.h.

// The code object holds gfx950 kernels only: any other device is "no usable device", not a launch error.
// (Cached per device id; a racing first call computes the same value.)  dev_out may be null.
int check_device(int *dev_out) {
  static std::atomic<int> arch_state[64];  // 0 unknown, 1 gfx950, -1 something else
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) {
    (void)hipGetLastError();
    return TSDF_ERR_NO_DEVICE;
  }
  if (dev_out) *dev_out = dev;
  if (dev < 0 || dev >= 64) return TSDF_OK;  // beyond the cache: let the launch decide
  int st = arch_state[dev].load(std::memory_order_relaxed);
  if (st == 0) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
      (void)hipGetLastError();
      return TSDF_ERR_NO_DEVICE;
    }
    st = strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : -1;
    arch_state[dev].store(st, std::memory_order_relaxed);
  }
  return st == 1 ? TSDF_OK : TSDF_ERR_NO_DEVICE;
}

// The CU count (> 0) of a device check_device accepts, or a negative tsdf_status: a device that reports no CUs is no
// usable device either.  Cached like the check; a device id beyond the cache is asked every time.
[[maybe_unused]] int device_cus() {
  static std::atomic<int> cached[64];  // 0 unknown
  int dev = 0;
  const int rc = check_device(&dev);
  if (rc != TSDF_OK) return rc;
  const bool in_cache = dev >= 0 && dev < 64;
  int cus = in_cache ? cached[dev].load(std::memory_order_relaxed) : 0;
  if (cus == 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
      (void)hipGetLastError();
      return TSDF_ERR_NO_DEVICE;
    }
    if (cus <= 0) return TSDF_ERR_NO_DEVICE;
    if (in_cache) cached[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

// what an entry returns once its kernel is queued
int launched() { return hipGetLastError() == hipSuccess ? TSDF_OK : TSDF_ERR_LAUNCH; }

// p is not a multiple of mask + 1 (mask: 1, 3, 7 or 15)
bool misaligned(const void *p, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(p) & mask) != 0; }

// R is not a resolution an extension voxelizes or places at (include/tsdf.h: tsdf_resolution_supported)
[[maybe_unused]] bool bad_res(int R) { return R < 4 || R > 128 || R % 4 != 0; }
