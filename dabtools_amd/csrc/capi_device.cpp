// capi_device.cpp — the entries of the C ABI (include/dabhip.h) about a device rather than a handle: how many there are and which, device and
// page-locked host memory for callers that bring no GPU runtime of their own, the copy ceiling, and the device-side modulator's shim.
#include <cstdio>
#include <string>

#include "capi_detail.hpp"
#include "engine.hpp"
#include "kernels.hpp"

using namespace dabhip;

extern "C" int dabhip_device_count(void)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// which physical device an index is: PCI bus id ("0000:c1:00.0") and marketing name -- what a multi-rank run records per rank, so that N ranks can be
// shown to have sat on N distinct GPUs (bench.py: ranks[].device)
extern "C" int dabhip_device_identity(int device, char* bus_id, int cap_bus, char* name, int cap_name)
{
  if (!bus_id || cap_bus < 16 || !name || cap_name < 2) { set_error("device_identity: buffers too small"); return -1; }
  hipDeviceProp_t prop;
  if (hipDeviceGetPCIBusId(bus_id, cap_bus, device) != hipSuccess || hipGetDeviceProperties(&prop, device) != hipSuccess) {
    (void)hipGetLastError();
    set_error("device_identity: no such device: " + std::to_string(device));
    return -1;
  }
  std::snprintf(name, static_cast<size_t>(cap_name), "%s", prop.name);
  return 0;
}

extern "C" int dabhip_stream_ceiling(int device, size_t bytes, int reps, double* gbs)
{
  if (!gbs) { set_error("stream_ceiling: null argument"); return -1; }
  if (dabhip::stream_ceiling(device, bytes, reps, gbs) != 0) { set_error("stream_ceiling: allocation or launch failed"); return -1; }
  return 0;
}

// device memory for callers that bring no GPU runtime of their own (the batch entries take device pointers)
extern "C" void* dabhip_device_alloc(size_t nbytes, int device)
{
  void* p = nullptr;
  if (hipSetDevice(device) != hipSuccess || hipMalloc(&p, nbytes ? nbytes : 1) != hipSuccess) { set_error("device_alloc: hipMalloc of " + std::to_string(nbytes) + " bytes failed"); return nullptr; }
  return p;
}
extern "C" void dabhip_device_free(void* p) { if (p) (void)hipFree(p); }
extern "C" int dabhip_device_copy(void* dst, const void* src, size_t nbytes, int to_device)
{
  if (!dst || !src) { set_error("device_copy: null argument"); return -1; }
  if (blocking_copy(dst, src, nbytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost) != hipSuccess) { set_error("device_copy: hipMemcpy failed"); return -1; }
  return 0;
}

// page-locked host memory for the segments handed to dabhip_stream_feed (read the next one while this one decodes)
extern "C" void* dabhip_host_alloc(size_t nbytes)
{
  void* p = nullptr;
  if (hipHostMalloc(&p, nbytes, hipHostMallocDefault) != hipSuccess) { set_error("host_alloc: hipHostMalloc failed"); return nullptr; }
  return p;
}
extern "C" void dabhip_host_free(void* p) { if (p) (void)hipHostFree(p); }

// ---- device-side modulator (k_synth.hip) ------------------------------------------------------
namespace dabhip { int synth_generate_device(const dabhip_synth_cfg* cfgs, int nstreams, int ntf, uint8_t* const* iq, int device); }
extern "C" int dabhip_synth_generate_device(const dabhip_synth_cfg* cfgs, int nstreams, int ntf, uint8_t* const* iq, int device)
{
  return dabhip::synth_generate_device(cfgs, nstreams, ntf, iq, device);
}
