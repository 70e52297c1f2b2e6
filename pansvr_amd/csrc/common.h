// common.h -- what the host-side translation units of libpsvr_engine.so share: error plumbing, the device buffer, and the scaffold of a
// "service call" (a C ABI function that owns a process-wide stream and device buffers: bgzf.hip, deflate_wave.hip, inflate.hip, sort.hip)
#pragma once
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <mutex>
#include <string>
#include "../../include/psvr_engine.h"

namespace psvr {

std::string &last_error_ref();

inline int set_error(int code, const char *fmt, ...)
{
	char buf[1024];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	last_error_ref() = buf;
	return code;
}

#define PSVR_HIP(call)                                                                        \
	do {                                                                                      \
		hipError_t e_ = (call);                                                               \
		if (e_ != hipSuccess)                                                                 \
			return psvr::set_error(PSVR_ERR_DEVICE, "%s failed: %s (%s:%d)", #call,           \
			                       hipGetErrorString(e_), __FILE__, __LINE__);                \
	} while (0)

// RAII device buffer (plain hipMalloc; sized for 288 GB HBM, no pooling needed at this level)
struct DevBuf {
	void *p = nullptr;
	size_t bytes = 0;
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	~DevBuf() { release(); }
	void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
	hipError_t alloc(size_t n)
	{
		release();
		if (n == 0) n = 16;
		hipError_t e = hipMalloc(&p, n);
		if (e == hipSuccess) bytes = n;
		else p = nullptr;
		return e;
	}
	hipError_t ensure(size_t n) { return n <= bytes ? hipSuccess : alloc(n + n / 4); }
	template <class T> T *as() const { return (T *)p; }
};

// The process-wide state of a service call: one caller at a time (mu), on the stream of the device it was last bound to.  The owner
// derives its context from it and keeps there what an asynchronous copy touches on the host, so that it lives as long as the stream.
struct DeviceService {
	std::mutex mu;
	int device = -1;
	hipStream_t stream = nullptr;
	// Makes `dev` current; when it is not the bound one: release() frees the owner's DevBufs, the stream is made anew (lowest_priority: an
	// engine launch that becomes ready while a call runs is not kept waiting behind it), setup() does what the owner needs once per device
	// (a hipError_t).  The device is recorded only once all of that has succeeded: after a failure the next call starts over.
	template <class Release, class Setup> int bind(int dev, bool lowest_priority, Release release, Setup setup)
	{
		PSVR_HIP(hipSetDevice(dev));
		if (device == dev) return PSVR_OK;
		device = -1;
		release();
		if (stream) (void)hipStreamDestroy(stream), stream = nullptr;
		int least = 0, greatest = 0;                                     // (0: the default priority)
		if (lowest_priority) PSVR_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
		PSVR_HIP(hipStreamCreateWithPriority(&stream, hipStreamNonBlocking, least));
		PSVR_HIP(setup());
		device = dev;
		return PSVR_OK;
	}
	template <class Release> int bind(int dev, bool lowest_priority, Release release) { return bind(dev, lowest_priority, release, [] { return hipSuccess; }); }
};

// Between a call's first asynchronous operation and its last wait: an error return in between leaves nothing in flight that reads the
// caller's input or writes its output.  Declared after the buffers the stream touches; disarmed before the wait that ends the call.
struct StreamDrain {
	hipStream_t s;
	bool armed = true;
	~StreamDrain() { if (armed) (void)hipStreamSynchronize(s); }
};

} // namespace psvr
