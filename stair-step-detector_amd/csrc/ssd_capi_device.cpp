/*
 * ssd_capi_device.cpp — the entry points of include/ssd_hip.h that take no handle but call HIP: the device count, pinned host memory,
 * plain device memory, a device's report and the binding of a thread to its CPUs.  Plain C++ like ssd_host.cpp.  Of ssd_capi.h it uses
 * HIP_TRY and hip_fail, of ssd_capi.hip nothing, and no ssd_handle.
 */
#include "ssd_capi.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>
#include <sched.h>

int ssd_device_count(void)
{
  int n = 0;
  if(hipGetDeviceCount(&n) != hipSuccess)
    return 0;
  return n;
}

/* pinned host memory for frames (DMA without a staging copy) */
int ssd_host_alloc(size_t bytes, void **ptr)
{
  if(!ptr || bytes == 0)
    return fail(SSD_E_ARG, "ssd_host_alloc: bad argument");
  if(ssd_device_count() <= 0)
    return fail(SSD_E_NODEVICE, "ssd_host_alloc: no HIP device");
  *ptr = nullptr;
  const hipError_t e = hipHostMalloc(ptr, bytes, hipHostMallocDefault);
  if(e != hipSuccess)
    return hip_fail(e, "hipHostMalloc: ");
  return SSD_OK;
}

int ssd_host_free(void *ptr)
{
  if(ptr)
    HIP_TRY(hipHostFree(ptr));
  return SSD_OK;
}

/* ---- plain device-memory helpers --------------------------------------------- */

int ssd_device_alloc(int device, size_t bytes, void **d_ptr)
{
  if(!d_ptr)
    return fail(SSD_E_ARG, "ssd_device_alloc: null");
  if(ssd_device_count() <= 0)
    return fail(SSD_E_NODEVICE, "ssd_device_alloc: no HIP device");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMalloc(d_ptr, bytes));
  return SSD_OK;
}
int ssd_device_free(int device, void *d_ptr)
{
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipFree(d_ptr));
  return SSD_OK;
}
int ssd_device_upload(int device, void *d_dst, const void *src, size_t bytes)
{
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice));
  return SSD_OK;
}
int ssd_device_download(int device, void *dst, const void *d_src, size_t bytes)
{
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost));
  return SSD_OK;
}
int ssd_device_sync(int device)
{
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  return SSD_OK;
}

namespace
{
/* first line of a sysfs attribute, without the newline; empty when it cannot be read */
std::string sysfs_line(const std::string &path)
{
  std::ifstream f(path);
  std::string s;
  if(f)
    std::getline(f, s);
  return s;
}
/* "0-15,128-143" -> CPU numbers; anything malformed ends the list there */
std::vector<int> parse_cpu_list(const std::string &list)
{
  std::vector<int> cpus;
  const char *p = list.c_str();
  while(*p)
  {
    char *end = nullptr;
    const long a = std::strtol(p, &end, 10);
    if(end == p || a < 0)
      break;
    long b = a;
    p = end;
    if(*p == '-')
    {
      b = std::strtol(p + 1, &end, 10);
      if(end == p + 1 || b < a)
        break;
      p = end;
    }
    for(long c = a; c <= b && cpus.size() < 4096; c++)
      cpus.push_back(static_cast<int>(c));
    if(*p == ',')
      p++;
    else
      break;
  }
  return cpus;
}
} // namespace

/* the device's report, and (full != nullptr) its local CPU list as sysfs spells it - the report's field holds 255 characters of it */
static int device_info_impl(int device, ssd_device_info *out, std::string *full)
{
  if(!out)
    return fail(SSD_E_ARG, "ssd_device_info_get: null");
  const int n = ssd_device_count();
  if(n <= 0)
    return fail(SSD_E_NODEVICE, "ssd_device_info_get: no HIP device");
  if(device < 0 || device >= n)
    return fail(SSD_E_ARG, "ssd_device_info_get: device index out of range");
  std::memset(out, 0, sizeof(*out));
  out->numa_node = -1;
  HIP_TRY(hipDeviceGetPCIBusId(out->pci_bus_id, static_cast<int>(sizeof(out->pci_bus_id)), device));
  for(char *c = out->pci_bus_id; *c; c++)
    if(*c >= 'A' && *c <= 'F')
      *c = static_cast<char>(*c - 'A' + 'a');                 /* sysfs spells bus ids in lower case */
  hipUUID uuid;
  hipDevice_t dev;
  if(hipDeviceGet(&dev, device) == hipSuccess && hipDeviceGetUuid(&uuid, dev) == hipSuccess)
  {
    static const char hex[] = "0123456789abcdef";
    for(int i = 0; i < 16; i++)
    {
      const unsigned char b = static_cast<unsigned char>(uuid.bytes[i]);
      out->uuid[2 * i] = hex[b >> 4];
      out->uuid[2 * i + 1] = hex[b & 15];
    }
  }
  else
    (void)hipGetLastError();
  const std::string dir = std::string("/sys/bus/pci/devices/") + out->pci_bus_id + "/";
  const std::string node = sysfs_line(dir + "numa_node");
  if(!node.empty())
    out->numa_node = std::atoi(node.c_str());
  const std::string cpus = sysfs_line(dir + "local_cpulist");
  std::snprintf(out->cpu_list, sizeof(out->cpu_list), "%s", cpus.c_str());
  out->n_local_cpus = static_cast<int32_t>(parse_cpu_list(cpus).size());
  if(full)
    *full = cpus;
  return SSD_OK;
}

int ssd_device_info_get(int device, ssd_device_info *out)
{
  return device_info_impl(device, out, nullptr);
}

int ssd_bind_thread_to_device(int device)
{
  ssd_device_info info;
  std::string list;               /* the whole sysfs line: the report's copy may end in the middle of a number ("128-143" cut to "12") */
  const int rc = device_info_impl(device, &info, &list);
  if(rc != SSD_OK)
    return rc;
  const std::vector<int> cpus = parse_cpu_list(list);
  if(cpus.empty())
    return 0;
  cpu_set_t *set = CPU_ALLOC(4096);
  if(!set)
    return fail(SSD_E_NOMEM, "ssd_bind_thread_to_device: CPU_ALLOC");
  const size_t bytes = CPU_ALLOC_SIZE(4096);
  /* only CPUs this thread may run on (a container's cpuset can be narrower than the node): an empty intersection changes nothing */
  cpu_set_t *allowed = CPU_ALLOC(4096);
  int bound = 0;
  if(allowed && sched_getaffinity(0, bytes, allowed) == 0)
  {
    CPU_ZERO_S(bytes, set);
    for(int c : cpus)
      if(c < 4096 && CPU_ISSET_S(c, bytes, allowed))
      {
        CPU_SET_S(c, bytes, set);
        bound++;
      }
    if(bound > 0 && sched_setaffinity(0, bytes, set) != 0)
      bound = 0;
  }
  if(allowed) CPU_FREE(allowed);
  CPU_FREE(set);
  return bound;
}

