// context.hip -- the device context (context.h): its life, its options, and the services every other unit leans on -- the
// device binding, the table cache, the scratch slots, the pool, the staging ring, the side lane, the fork lanes, the timer.
// Everything tvm_ctx_destroy has to give back is created in this file.  One kernel: k_pow_table.
#define TVM_MUL_CARRY_FORM 0   // k_pow_table in the form it has always been compiled in (beside the transforms: ntt.hip)
#include <cstring>
#include <new>

#include "context.h"

#define TVM_ABI_VERSION 1

namespace tvm {

__global__ void k_pow_table(u64 base, u64 count, u64 scale, u64* out) {
    u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = bfe_mul(scale, bfe_pow(base, i));
}

int set_error(tvm_ctx* c, int code, const char* what) {
    if (c) c->last_error = what;
    return code;
}

bool bind_device(tvm_ctx* c) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == c->device) return true;
    return hipSetDevice(c->device) == hipSuccess;
}

// The device's compute units (256 on an MI355X); 0 where it reports none -- the CPU emulation has no such thing, and a driver that
// refuses the question leaves the caller at the value that asks for nothing.
static u64 compute_units(int device) {
#ifdef TVM_EMU
    (void)device;
    return 0;
#else
    int n = 0;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n > 0 ? (u64)n : 0;
#endif
}

// ---- the table cache
u64* cached_table(tvm_ctx* c, TableKind kind, u64 a, u64 b, u64 d, u64 words, bool* is_new) {
    const auto key = std::make_tuple(kind, a, b, d);
    *is_new = false;
    auto it = c->tables.find(key);
    if (it != c->tables.end()) return it->second;
    u64* t = nullptr;
    if (!bind_device(c) || hipMalloc((void**)&t, (words ? words : 1) * sizeof(u64)) != hipSuccess) return nullptr;
    c->tables[key] = t;
    *is_new = true;
    return t;
}
void drop_cached_table(tvm_ctx* c, TableKind kind, u64 a, u64 b, u64 d) {
    auto it = c->tables.find(std::make_tuple(kind, a, b, d));
    if (it == c->tables.end()) return;
    (void)hipFree(it->second);
    c->tables.erase(it);
}

const u64* pow_table(tvm_ctx* c, u64 base, u64 count, u64 scale) {
    bool is_new = false;
    u64* d = cached_table(c, TableKind::Powers, base, count, scale, count, &is_new);
    if (is_new) {
        const int bs = 256;
        TVM_LAUNCH(k_pow_table, dim3((unsigned)((count + bs - 1) / bs)), dim3(bs), 0, c->stream, base, count, scale, d);
    }
    return d;
}

// ---- the scratch slots
void* scratch(tvm_ctx* c, Scratch which, size_t bytes) {
    const int slot = (int)which;
    if (c->scratch_bytes[slot] < bytes) {
        if (c->scratch[slot]) {
            (void)hipStreamSynchronize(c->stream);
            (void)hipFree(c->scratch[slot]);
            c->scratch[slot] = nullptr;
            c->scratch_bytes[slot] = 0;
        }
        void* p = nullptr;
        if (!bind_device(c) || hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        c->scratch[slot] = p;
        c->scratch_bytes[slot] = bytes;
    }
    return c->scratch[slot];
}

const u64* stage_small(tvm_ctx* c, Scratch slot, const u64* h, size_t words) {
    u64* d = (u64*)scratch(c, slot, (words ? words : 1) * sizeof(u64));
    if (!d) return nullptr;
    if (h2d_small(c, d, h, words * sizeof(u64)) != TVM_OK) return nullptr;   // (h may be a caller temporary)
    return d;
}

// ---- the pool
static size_t pool_round(size_t bytes) {
    const size_t g = bytes < (1u << 20) ? 256 : (2u << 20);
    return (bytes + g - 1) / g * g;
}
void* pool_alloc(tvm_ctx* c, size_t bytes) {
    const size_t want = pool_round(bytes ? bytes : 1);
    auto it = c->pool_free.lower_bound(want);
    if (it != c->pool_free.end() && it->first <= want + want / 4) {  // at most 25 % slack
        void* p = it->second;
        c->pool_live[p] = it->first;
        c->pool_free.erase(it);
        return p;
    }
    void* p = nullptr;
    if (!bind_device(c)) return nullptr;
    if (c->pool_limit && c->pool_bytes + want > c->pool_limit) {
        pool_trim(c);  // cached blocks count against the limit: give them back first
        if (c->pool_bytes + want > c->pool_limit) return nullptr;
    }
    if (hipMalloc(&p, want) != hipSuccess) {
        (void)hipGetLastError();
        pool_trim(c);
        if (hipMalloc(&p, want) != hipSuccess) {
            (void)hipGetLastError();
            return nullptr;
        }
    }
    c->pool_live[p] = want;
    c->pool_bytes += want;
    return p;
}
void pool_release(tvm_ctx* c, void* p) {
    if (!p) return;
    auto it = c->pool_live.find(p);
    if (it == c->pool_live.end()) {  // not ours (should not happen): hand it to the driver
        (void)hipStreamSynchronize(c->stream);
        (void)hipFree(p);
        return;
    }
    c->pool_free.emplace(it->second, p);
    c->pool_live.erase(it);
}
void pool_trim(tvm_ctx* c) {
    if (c->pool_free.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto& kv : c->pool_free) {
        (void)hipFree(kv.second);
        c->pool_bytes -= kv.first;
    }
    c->pool_free.clear();
}
size_t pool_available(tvm_ctx* c, size_t* device_total) {
    size_t free_b = 0, total_b = 0;
    if (!bind_device(c) || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
    size_t cached = 0;
    for (const auto& kv : c->pool_free) cached += kv.first;
    size_t avail = free_b + cached;
    if (c->pool_limit) {
        const size_t live = c->pool_bytes - cached;
        avail = live >= c->pool_limit ? 0 : (avail < c->pool_limit - live ? avail : c->pool_limit - live);
    }
    if (device_total) *device_total = total_b;
    return avail;
}

// ---- the staging ring
int h2d_small(tvm_ctx* c, void* d, const void* h, size_t bytes) {
    if (!bytes) return TVM_OK;
    constexpr size_t RING = (size_t)4 << 20;
    if (!c->pin && !c->pin_unavailable) {
        void* p = nullptr;
        if (bind_device(c) && hipHostMalloc(&p, RING, 0) == hipSuccess) {
            c->pin = (char*)p;
            c->pin_bytes = RING;
        } else {
            (void)hipGetLastError();
            c->pin_unavailable = true;
        }
    }
    if (!c->pin || bytes > c->pin_bytes / 4) {
        TVM_HIP_CHECK(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
        TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        return TVM_OK;
    }
    const size_t need = (bytes + 63) & ~(size_t)63;
    if (c->pin_head + need > c->pin_bytes) {   // wrap: every copy out of the ring so far has been issued on this stream
        TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
        c->pin_head = 0;
    }
    char* slot = c->pin + c->pin_head;
    c->pin_head += need;
    std::memcpy(slot, h, bytes);
    TVM_HIP_CHECK(c, hipMemcpyAsync(d, slot, bytes, hipMemcpyHostToDevice, c->stream));
    return TVM_OK;
}

// ---- the fork lanes
bool fork_lanes(tvm_ctx* c) {
    if (c->fork_ready) return true;
    if (!bind_device(c)) return false;
    hipStream_t s[3] = {};
    hipEvent_t e[4] = {};
    bool ok = true;
    for (int k = 0; k < 3 && ok; k++) ok = hipStreamCreateWithFlags(&s[k], hipStreamNonBlocking) == hipSuccess;
    for (int k = 0; k < 4 && ok; k++) ok = hipEventCreateWithFlags(&e[k], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        for (hipStream_t x : s)
            if (x) hipStreamDestroy(x);
        for (hipEvent_t x : e)
            if (x) hipEventDestroy(x);
        return false;
    }
    for (int k = 0; k < 3; k++) c->fork[k] = s[k], c->fork_done[k] = e[k];
    c->fork_ready = e[3];
    return true;
}

// ---- the side lane (include/triton_hip.h)
static_assert(TVM_SIDE_SLOTS == 16, "tvm_ctx::side_done has sixteen slots");
static bool side_lane(tvm_ctx* c) {
    if (c->side) return true;
    if (!bind_device(c)) return false;
    hipStream_t s = nullptr;
    hipEvent_t ready = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return false;
    if (hipEventCreateWithFlags(&ready, hipEventDisableTiming) != hipSuccess) {
        hipStreamDestroy(s);
        return false;
    }
    c->side = s;
    c->side_ready = ready;
    return true;
}
}  // namespace tvm

using namespace tvm;

extern "C" {

int32_t tvm_abi_version(void) { return TVM_ABI_VERSION; }

const char* tvm_status_string(int32_t s) {
    switch (s) {
        case TVM_OK: return "ok";
        case TVM_ERR_INVALID_ARGUMENT: return "invalid argument";
        case TVM_ERR_OUT_OF_MEMORY: return "device out of memory";
        case TVM_ERR_DEVICE: return "HIP runtime error";
        case TVM_ERR_UNSUPPORTED: return "unsupported size or configuration";
        case TVM_NOT_APPLICABLE: return "not applicable to these arguments";
        default: return "unknown status";
    }
}

int32_t tvm_ctx_create(int32_t device, void* hip_stream, tvm_ctx** out) {
    if (!out) return TVM_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return TVM_ERR_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return TVM_ERR_DEVICE;
    tvm_ctx* c = new (std::nothrow) tvm_ctx();
    if (!c) return TVM_ERR_OUT_OF_MEMORY;
    c->device = device;
    c->lde_pass1_workgroups = compute_units(device);   // LDE pass 1 starts with a workgroup per compute unit (context.h)
    if (hip_stream) {
        c->stream = (hipStream_t)hip_stream;
    } else {
        if (hipStreamCreate(&c->stream) != hipSuccess) {
            delete c;
            return TVM_ERR_DEVICE;
        }
        c->owns_stream = true;
    }
    *out = c;
    return TVM_OK;
}

void tvm_ctx_destroy(tvm_ctx* c) {
    if (!c) return;
    hipStreamSynchronize(c->stream);
    for (auto& kv : c->tables) hipFree(kv.second);
    for (void* p : c->scratch)
        if (p) hipFree(p);
    for (auto& kv : c->pool_free) hipFree(kv.second);
    for (auto& kv : c->pool_live) hipFree(kv.first);
    if (c->ev_start) hipEventDestroy(c->ev_start);
    if (c->ev_stop) hipEventDestroy(c->ev_stop);
    if (c->side) {
        hipStreamSynchronize(c->side);
        hipStreamDestroy(c->side);
    }
    if (c->side_ready) hipEventDestroy(c->side_ready);
    for (hipStream_t s : c->fork)
        if (s) {
            hipStreamSynchronize(s);
            hipStreamDestroy(s);
        }
    if (c->fork_ready) hipEventDestroy(c->fork_ready);
    for (hipEvent_t e : c->fork_done)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->side_done)
        if (e) hipEventDestroy(e);
    if (c->pin) hipHostFree(c->pin);
    if (c->owns_stream) hipStreamDestroy(c->stream);
    delete c;
}

const char* tvm_last_error(const tvm_ctx* c) { return c ? c->last_error.c_str() : "null context"; }

int32_t tvm_sync(tvm_ctx* c) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return TVM_OK;
}
int32_t tvm_malloc(tvm_ctx* c, size_t bytes, void** d_ptr) {
    if (!c || !d_ptr) return TVM_ERR_INVALID_ARGUMENT;
    *d_ptr = pool_alloc(c, bytes);
    if (!*d_ptr) return set_error(c, TVM_ERR_OUT_OF_MEMORY, "tvm_malloc");
    return TVM_OK;
}
int32_t tvm_free(tvm_ctx* c, void* d_ptr) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    pool_release(c, d_ptr);
    return TVM_OK;
}
int32_t tvm_ctx_set_memory_limit(tvm_ctx* c, size_t bytes) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    c->pool_limit = bytes;
    return TVM_OK;
}
int32_t tvm_ctx_memory_held(const tvm_ctx* c, size_t* bytes) {
    if (!c || !bytes) return TVM_ERR_INVALID_ARGUMENT;
    *bytes = c->pool_bytes;
    return TVM_OK;
}
int32_t tvm_ctx_memory_info(const tvm_ctx* c, size_t* available_bytes, size_t* device_total_bytes) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    int cur = -1;
    (void)hipGetDevice(&cur);
    size_t total = 0;
    const size_t avail = pool_available(const_cast<tvm_ctx*>(c), &total);   // (binds the context's device; reads the pool only)
    if (cur >= 0 && cur != c->device) (void)hipSetDevice(cur);
    if (!total) return TVM_ERR_DEVICE;
    if (available_bytes) *available_bytes = avail;
    if (device_total_bytes) *device_total_bytes = total;
    return TVM_OK;
}
int32_t tvm_ctx_set_option(tvm_ctx* c, int32_t option, uint64_t value) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    if (option == TVM_OPTION_AIR_VALID_TRACE) {
        c->air_valid_trace = value != 0;
        return TVM_OK;
    }
    if (option == TVM_OPTION_LDE_CHUNK_COLUMNS) {
        if (value > 4096) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "TVM_OPTION_LDE_CHUNK_COLUMNS: at most 4096");
        c->lde_chunk_columns = (int)value;
        return TVM_OK;
    }
    if (option == TVM_OPTION_LDE_PASS2_TILES) {
        c->lde_pass2_tiles = value ? 1 : 0;
        return TVM_OK;
    }
    if (option == TVM_OPTION_LDE_PASS2_SCALE_ABSORBED) {
        c->lde_pass2_scale_absorbed = value != 0;
        return TVM_OK;
    }
    if (option == TVM_OPTION_LDE_PASS1_WORKGROUPS) {
        if (value > (1ull << 30)) return set_error(c, TVM_ERR_INVALID_ARGUMENT, "TVM_OPTION_LDE_PASS1_WORKGROUPS: at most 2^30");
        c->lde_pass1_workgroups = value;
        return TVM_OK;
    }
    if (option == TVM_OPTION_MERKLE_SUBTREES) {
        c->merkle_subtrees = value != 0;
        return TVM_OK;
    }
    if (option == TVM_OPTION_AIR_FORK_MAX_WORKGROUPS) {
        c->air_fork_max_workgroups = value;
        return TVM_OK;
    }
    if (option == TVM_OPTION_AIR_REMAINDER_COSET) {
        c->air_remainder_coset = value != 0;
        return TVM_OK;
    }
    if (option == TVM_OPTION_AIR_REMAINDER_MIN_ROWS) {
        c->air_remainder_min_rows = value ? value : 1ull << 18;
        return TVM_OK;
    }
    if (option == TVM_OPTION_AIR_CHECK_CHUNK_ROWS) {
        if (value && (!is_pow2(value) || value < TVM_RB || value > (1ull << 20)))
            return set_error(c, TVM_ERR_INVALID_ARGUMENT, "TVM_OPTION_AIR_CHECK_CHUNK_ROWS: a power of two in 16 .. 2^20");
        c->air_check_chunk_rows = value ? value : 1ull << 18;
        return TVM_OK;
    }
    if (option == TVM_OPTION_SEGMENTS_FROM_COEFFICIENTS) {
        c->segments_from_coefficients = value != 0;
        return TVM_OK;
    }
    if (option == TVM_OPTION_COMBINATION_FROM_COEFFICIENTS) {
        c->combination_from_coefficients = value != 0;
        return TVM_OK;
    }
    if (option == TVM_OPTION_MERKLE_MIN_WORKGROUPS) {
        c->merkle_min_workgroups = value ? value : 4096;
        return TVM_OK;
    }
    return set_error(c, TVM_ERR_INVALID_ARGUMENT, "unknown option");
}
int32_t tvm_ctx_get_option(const tvm_ctx* c, int32_t option, uint64_t* value) {
    if (!c || !value) return TVM_ERR_INVALID_ARGUMENT;
    switch (option) {
        case TVM_OPTION_LDE_PASS2_SCALE_ABSORBED: *value = c->lde_pass2_scale_absorbed; return TVM_OK;
        case TVM_OPTION_LDE_PASS1_WORKGROUPS: *value = c->lde_pass1_workgroups; return TVM_OK;
        case TVM_OPTION_SEGMENTS_FROM_COEFFICIENTS: *value = c->segments_from_coefficients; return TVM_OK;
        case TVM_OPTION_COMBINATION_FROM_COEFFICIENTS: *value = c->combination_from_coefficients; return TVM_OK;
        default: return TVM_ERR_INVALID_ARGUMENT;
    }
}
int32_t tvm_ctx_trim(tvm_ctx* c) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    pool_trim(c);
    return TVM_OK;
}
int32_t tvm_memcpy_h2d(tvm_ctx* c, void* d, const void* h, size_t bytes) {
    if (!c || (bytes && (!d || !h))) return TVM_ERR_INVALID_ARGUMENT;
    TVM_HIP_CHECK(c, hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return TVM_OK;
}
int32_t tvm_memcpy_d2h(tvm_ctx* c, void* h, const void* d, size_t bytes) {
    if (!c || (bytes && (!d || !h))) return TVM_ERR_INVALID_ARGUMENT;
    TVM_HIP_CHECK(c, hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    TVM_HIP_CHECK(c, hipStreamSynchronize(c->stream));
    return TVM_OK;
}
int32_t tvm_memcpy_d2d(tvm_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return TVM_ERR_INVALID_ARGUMENT;
    if (bytes) TVM_HIP_CHECK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
    return TVM_OK;
}
void* tvm_ctx_stream(const tvm_ctx* c) { return c ? (void*)c->stream : nullptr; }

void* tvm_ctx_side_stream(tvm_ctx* c) { return c && side_lane(c) ? (void*)c->side : nullptr; }
int32_t tvm_side_begin(tvm_ctx* c) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    if (!side_lane(c)) return tvm::set_error(c, TVM_ERR_DEVICE, "tvm_side_begin: no second stream");
    TVM_HIP_CHECK(c, hipEventRecord(c->side_ready, c->stream));
    TVM_HIP_CHECK(c, hipStreamWaitEvent(c->side, c->side_ready, 0));
    return TVM_OK;
}
int32_t tvm_side_memcpy_d2d(tvm_ctx* c, void* dst, const void* src, size_t bytes) {
    if (!c || (bytes && (!dst || !src))) return TVM_ERR_INVALID_ARGUMENT;
    if (!side_lane(c)) return tvm::set_error(c, TVM_ERR_DEVICE, "tvm_side_memcpy_d2d: no second stream");
    if (bytes) TVM_HIP_CHECK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->side));
    return TVM_OK;
}
int32_t tvm_side_mark(tvm_ctx* c, uint32_t slot) {
    if (!c || slot >= TVM_SIDE_SLOTS) return TVM_ERR_INVALID_ARGUMENT;
    if (!side_lane(c)) return tvm::set_error(c, TVM_ERR_DEVICE, "tvm_side_mark: no second stream");
    if (!c->side_done[slot]) TVM_HIP_CHECK(c, hipEventCreateWithFlags(&c->side_done[slot], hipEventDisableTiming));
    TVM_HIP_CHECK(c, hipEventRecord(c->side_done[slot], c->side));
    return TVM_OK;
}
int32_t tvm_side_wait(tvm_ctx* c, uint32_t slot) {
    if (!c || slot >= TVM_SIDE_SLOTS) return TVM_ERR_INVALID_ARGUMENT;
    if (c->side_done[slot]) TVM_HIP_CHECK(c, hipStreamWaitEvent(c->stream, c->side_done[slot], 0));   // (never marked: nothing to wait for)
    return TVM_OK;
}
int32_t tvm_side_sync(tvm_ctx* c) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    if (c->side) TVM_HIP_CHECK(c, hipStreamSynchronize(c->side));
    return TVM_OK;
}

int32_t tvm_timer_start(tvm_ctx* c) {
    if (!c) return TVM_ERR_INVALID_ARGUMENT;
    if (!c->ev_start) {
        TVM_HIP_CHECK(c, hipEventCreate(&c->ev_start));
        TVM_HIP_CHECK(c, hipEventCreate(&c->ev_stop));
    }
    TVM_HIP_CHECK(c, hipEventRecord(c->ev_start, c->stream));
    return TVM_OK;
}
int32_t tvm_timer_stop(tvm_ctx* c, float* ms) {
    if (!c || !ms || !c->ev_start) return TVM_ERR_INVALID_ARGUMENT;
    TVM_HIP_CHECK(c, hipEventRecord(c->ev_stop, c->stream));
    TVM_HIP_CHECK(c, hipEventSynchronize(c->ev_stop));
    TVM_HIP_CHECK(c, hipEventElapsedTime(ms, c->ev_start, c->ev_stop));
    return TVM_OK;
}
}  // extern "C"
