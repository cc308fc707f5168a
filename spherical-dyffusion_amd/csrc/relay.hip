// Relay hand-over between processes (ensemble.RelayComm(transport="peer")): an exported pool of state slots, its mapping in
// another process, and a copy on the SDMA engines (no CU, no kernel).  Host-side entry points only; nothing here launches.
#include <cstring>
#include "common.h"

static_assert(sizeof(hipIpcMemHandle_t) == 64, "sdy_relay_pool_create hands out 64-byte IPC handles");

// hipIpcGetMemHandle exports the allocation its pointer lies in: the pool is one hipMalloc of its own (never a
// suballocation of a caching allocator, whose handles would export a neighbour's memory as well), rounded up to 2 MiB.
static constexpr size_t SDY_POOL_ALIGN = size_t(2) << 20;

extern "C" int sdy_relay_pool_create(size_t slot_bytes, int n_slots, void** base, unsigned char handle[64]) {
  if (!base || !handle || slot_bytes == 0 || n_slots <= 0) return SDY_ERR_ARG;
  *base = nullptr;
  if (slot_bytes > (SIZE_MAX - SDY_POOL_ALIGN) / (size_t)n_slots) return SDY_ERR_ARG;
  const size_t bytes = (slot_bytes * (size_t)n_slots + SDY_POOL_ALIGN - 1) / SDY_POOL_ALIGN * SDY_POOL_ALIGN;
  void* p = nullptr;
  SDY_HIP_TRY(hipMalloc(&p, bytes));
  hipIpcMemHandle_t h;
  const hipError_t e = hipIpcGetMemHandle(&h, p);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return (int)e;
  }
  std::memcpy(handle, &h, sizeof(h));
  *base = p;
  return SDY_OK;
}

extern "C" int sdy_relay_pool_destroy(void* base) {
  if (!base) return SDY_ERR_ARG;
  SDY_HIP_TRY(hipFree(base));
  return SDY_OK;
}

extern "C" int sdy_ipc_open(const unsigned char handle[64], void** ptr) {
  if (!handle || !ptr) return SDY_ERR_ARG;
  *ptr = nullptr;
  hipIpcMemHandle_t h;
  std::memcpy(&h, handle, sizeof(h));
  SDY_HIP_TRY(hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess));
  return SDY_OK;
}

extern "C" int sdy_ipc_close(void* ptr) {
  if (!ptr) return SDY_ERR_ARG;
  SDY_HIP_TRY(hipIpcCloseMemHandle(ptr));
  return SDY_OK;
}

extern "C" int sdy_copy_nocu(void* dst, const void* src, size_t bytes, void* stream) {
  if (!dst || !src || bytes == 0) return SDY_ERR_ARG;
  SDY_HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDeviceNoCU, (hipStream_t)stream));
  return SDY_OK;
}
