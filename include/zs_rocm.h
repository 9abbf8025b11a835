/*
 * zs_rocm.h -- C ABI of libzsrocm.so, the MI355X (gfx950) backend for zpc's data-parallel hot path.
 *
 * Two groups of entry points:
 *
 *  (A) the reference's own C ABI (include/zensim/py_interop/, the `zpc_py_interop` target that Python
 *      `zpc_jit` binds through ctypes), re-exported 1:1 with `cuda` -> `rocm` in the symbol names:
 *      policy handles, launch__device, typed parallel primitives over `aosoa_iterator_port`s,
 *      Vector / TileVector / bht container handles.  Each declaration cites the file:line it replaces.
 *
 *  (B) `zs_rocm_*` entry points for work that in the reference only exists as C++ template
 *      instantiations inside user translation units (`pol(range(n), P2GTransfer{...})`,
 *      `tb.insert(key)` in a lambda, ...).  A C++ caller reaches them through the header-only face in
 *      include/zensim_rocm/; each declaration cites the functor it replaces.
 *
 * Conventions (same as the reference): every create returns a heap object owned by the
 * caller and released with the matching del_*; views are non-owning; functions return void and report
 * device errors by printing the first error per device to stderr and latching it
 * (zs_rocm_last_error), never by throwing across the ABI.  All device pointers are plain HIP device
 * pointers; no framework types appear in any signature.
 */
#ifndef ZS_ROCM_H
#define ZS_ROCM_H
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#  define ZS_ROCM_EXPORT __attribute__((visibility("default")))
#else
#  define ZS_ROCM_EXPORT
#endif

/* ======================================================================== (A) policy & launch */
/* zs::CudaExecutionPolicy (cuda/execution/ExecutionPolicy.cuh:345-911) -> RocmExecutionPolicy */
typedef struct zs_rocm_policy zs_rocm_policy;

/* py_interop/cuda/ExecutionPolicy.cpp:8-9 */
ZS_ROCM_EXPORT zs_rocm_policy *policy__device(void);
ZS_ROCM_EXPORT void del_policy__device(zs_rocm_policy *);
/* fluent setters of ExecutionPolicyInterface / CudaExecutionPolicy
 * (execution/ExecutionPolicy.hpp:110-126, cuda/execution/ExecutionPolicy.cuh:362-385).
 * Defaults: sync = 1, profile = 0, device = -1 (current), stream = -1 (null stream), block = 0. */
ZS_ROCM_EXPORT void zs_rocm_policy_sync(zs_rocm_policy *, int sync);
ZS_ROCM_EXPORT void zs_rocm_policy_profile(zs_rocm_policy *, int profile);
ZS_ROCM_EXPORT void zs_rocm_policy_device(zs_rocm_policy *, int procid);
ZS_ROCM_EXPORT void zs_rocm_policy_stream(zs_rocm_policy *, int streamid); /* -1 | 0..31 spare streams (cuda/Cuda.h:39,115-120) */
ZS_ROCM_EXPORT void zs_rocm_policy_listen(zs_rocm_policy *, int incomingProc, int incomingStreamid);
ZS_ROCM_EXPORT void zs_rocm_policy_shmem(zs_rocm_policy *, size_t bytes);
ZS_ROCM_EXPORT void zs_rocm_policy_block(zs_rocm_policy *, int tpb);
/* run on a stream owned by the caller (e.g. the framework's current stream); NULL restores streamid */
ZS_ROCM_EXPORT void zs_rocm_policy_external_stream(zs_rocm_policy *, void *hipStream);
ZS_ROCM_EXPORT void *zs_rocm_policy_get_stream(const zs_rocm_policy *); /* getStream(), :379 */
ZS_ROCM_EXPORT int zs_rocm_policy_should_sync(const zs_rocm_policy *);
ZS_ROCM_EXPORT void zs_rocm_policy_sync_ctx(const zs_rocm_policy *);   /* syncCtx(), :396-399 */
ZS_ROCM_EXPORT float zs_rocm_policy_last_elapsed_ms(const zs_rocm_policy *); /* profile(true): hipEvent pair */
/* latched error status of the device context (cuda/Cuda.h:291-312); 0 = hipSuccess */
ZS_ROCM_EXPORT int zs_rocm_last_error(int device);
ZS_ROCM_EXPORT void zs_rocm_clear_error(int device);
ZS_ROCM_EXPORT int zs_rocm_device_count(void);
ZS_ROCM_EXPORT int zs_rocm_current_device(void); /* the calling thread's HIP device (0 without a GPU) */
/* scratch memory for a caller-side kernel sequence on the policy's stream: the stream-ordered temporary of
 * get_temporary_memory_source(pol) (resource/cuda/ExecutionPolicy.cu:5-16, temporary_memory_resource::do_allocate /
 * do_deallocate, cuda/memory/Allocator.h:33-50 = cuMemAllocAsync / cuMemFreeAsync).  hipMallocAsync / hipFreeAsync on the
 * policy's stream: a block stays valid until it is handed back and never overlaps another live block or the scratch the
 * library's own primitives take. */
ZS_ROCM_EXPORT void *zs_rocm_policy_temporary(zs_rocm_policy *, size_t bytes);
ZS_ROCM_EXPORT void zs_rocm_policy_temporary_free(zs_rocm_policy *, void *ptr);
/* Vector::reset(byteVal) / TileVector::reset(pol, 0) on raw device memory: hipMemsetAsync on the policy's stream */
ZS_ROCM_EXPORT void zs_rocm_memset(zs_rocm_policy *, void *ptr, int byteVal, size_t bytes);
/* frees the grow-only per-stream arenas of the library's own per-call scratch (stand-in for streamMemFree, cuda/Cuda.cu:169-176) */
ZS_ROCM_EXPORT void zs_rocm_release_temporaries(void);

/* py_interop/cuda/ExecutionPolicy.cpp:11-39: launch a module function (hipFunction_t) over `dim`
 * threads, block 128, grid ceil(dim/128), on the policy's stream, sync if shouldSync() */
ZS_ROCM_EXPORT void launch__device(zs_rocm_policy *, void *kernel, size_t dim, void **args);

/* ======================================================================== (A) runtime compilation */
/* py_interop/cuda/Nvrtc.cpp:29-271 with hiprtc: cuda_compile_program / cuda_load_module / cuda_unload_module /
 * cuda_get_kernel / cuda_launch_kernel -> rocm_*.  `arch` is the gfx number (950); 0 takes it from the current device.
 * The output file is a code object; rocm_get_kernel returns the hipFunction_t that launch__device accepts.
 * rocm_compile_program returns 0 on success (hiprtcResult otherwise, (size_t)-1 if hiprtc cannot be loaded). */
ZS_ROCM_EXPORT size_t rocm_compile_program(const char *src, int arch, const char *include_dir, bool debug, bool verbose,
                                           bool verify_fp, bool fast_math, const char *output_path);
ZS_ROCM_EXPORT void *rocm_load_module(void *pol, const char *path);
ZS_ROCM_EXPORT void rocm_unload_module(void *pol, void *module);
ZS_ROCM_EXPORT void *rocm_get_kernel(void *pol, void *module, const char *name);
ZS_ROCM_EXPORT size_t rocm_launch_kernel(void *context, void *kernel, size_t dim, void **args, void *stream);

/* ======================================================================== (A) iterator ABI */
/* py_interop/GenericIterator.hpp:11-16: element address =
 *   base + ((((idx >> numTileBits) * numChns) << numTileBits) | (idx & tileMask));
 * AoS form: numTileBits = tileMask = 0.  Passed BY VALUE. */
#define ZS_ROCM_DECL_PORT(T, NAME)                                   \
  typedef struct {                                                   \
    T *base;                                                         \
    uint32_t idx, numTileBits, tileMask, numChns;                    \
  } NAME;
ZS_ROCM_DECL_PORT(int, aosoa_iterator_int_1)
ZS_ROCM_DECL_PORT(const int, aosoa_iterator_const_int_1)
ZS_ROCM_DECL_PORT(float, aosoa_iterator_float_1)
ZS_ROCM_DECL_PORT(const float, aosoa_iterator_const_float_1)
ZS_ROCM_DECL_PORT(double, aosoa_iterator_double_1)
ZS_ROCM_DECL_PORT(const double, aosoa_iterator_const_double_1)
/* aosoa_iterator_port<T, 3>: same POD, dereferences to 3 components `tileMask + 1` elements apart (GenericIterator.hpp:96-104);
 * the AoS form has numChns = 3 (element i at base + 3 i) */
ZS_ROCM_DECL_PORT(int, aosoa_iterator_int_3)
ZS_ROCM_DECL_PORT(const int, aosoa_iterator_const_int_3)
ZS_ROCM_DECL_PORT(float, aosoa_iterator_float_3)
ZS_ROCM_DECL_PORT(const float, aosoa_iterator_const_float_3)
ZS_ROCM_DECL_PORT(double, aosoa_iterator_double_3)
ZS_ROCM_DECL_PORT(const double, aosoa_iterator_const_double_3)

/* ======================================================================== (A) parallel primitives */
/* py_interop/cuda/ExecutionPolicy.cpp:41-131 (ZS_DEFINE_PARALLEL_PRIMITIVES for int, float, double).
 * reduce: out[0] = fold(op, init, [first,last)) with init = 0 / 1 / numeric max / numeric lowest;
 * scans with init = identity; merge sort = stable in-place sort by `<` (`:99-111`; pair form permutes int values);
 * radix sort over all key bits (integral T only, as in the reference). */
#define ZS_ROCM_DECL_PRIMITIVES(T)                                                                          \
  ZS_ROCM_EXPORT void reduce_sum__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_const_##T##_1 first,        \
                                               aosoa_iterator_const_##T##_1 last, aosoa_iterator_##T##_1);  \
  ZS_ROCM_EXPORT void reduce_prod__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_const_##T##_1 first,       \
                                                aosoa_iterator_const_##T##_1 last, aosoa_iterator_##T##_1); \
  ZS_ROCM_EXPORT void reduce_min__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_const_##T##_1 first,        \
                                               aosoa_iterator_const_##T##_1 last, aosoa_iterator_##T##_1);  \
  ZS_ROCM_EXPORT void reduce_max__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_const_##T##_1 first,        \
                                               aosoa_iterator_const_##T##_1 last, aosoa_iterator_##T##_1);  \
  ZS_ROCM_EXPORT void exclusive_scan_sum__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_const_##T##_1,      \
                                                       aosoa_iterator_const_##T##_1, aosoa_iterator_##T##_1); \
  ZS_ROCM_EXPORT void exclusive_scan_prod__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_const_##T##_1,     \
                                                        aosoa_iterator_const_##T##_1, aosoa_iterator_##T##_1); \
  ZS_ROCM_EXPORT void inclusive_scan_sum__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_const_##T##_1,      \
                                                       aosoa_iterator_const_##T##_1, aosoa_iterator_##T##_1); \
  ZS_ROCM_EXPORT void inclusive_scan_prod__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_const_##T##_1,     \
                                                        aosoa_iterator_const_##T##_1, aosoa_iterator_##T##_1); \
  ZS_ROCM_EXPORT void merge_sort__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_##T##_1 first,              \
                                               aosoa_iterator_##T##_1 last);                                \
  ZS_ROCM_EXPORT void merge_sort_pair__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_##T##_1 keys,          \
                                                    aosoa_iterator_int_1 vals, size_t count);               \
  ZS_ROCM_EXPORT void radix_sort__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_##T##_1 first,              \
                                               aosoa_iterator_##T##_1 last, aosoa_iterator_##T##_1 out);    \
  ZS_ROCM_EXPORT void radix_sort_pair__rocm_##T##_1(zs_rocm_policy *, aosoa_iterator_##T##_1 keysIn,        \
                                                    aosoa_iterator_int_1 valsIn, aosoa_iterator_##T##_1 keysOut, \
                                                    aosoa_iterator_int_1 valsOut, size_t count);
ZS_ROCM_DECL_PRIMITIVES(int)
ZS_ROCM_DECL_PRIMITIVES(float)
ZS_ROCM_DECL_PRIMITIVES(double)

/* (B) primitives on contiguous device arrays with the full argument set of the C++ face
 * (execution/ExecutionPolicy.hpp:698-781: init, bit window [sbit, ebit), other key widths). */
ZS_ROCM_EXPORT void zs_rocm_reduce_i32(zs_rocm_policy *, const int32_t *in, size_t n, int32_t *out, int32_t init, int op);
ZS_ROCM_EXPORT void zs_rocm_reduce_i64(zs_rocm_policy *, const int64_t *in, size_t n, int64_t *out, int64_t init, int op);
ZS_ROCM_EXPORT void zs_rocm_reduce_f32(zs_rocm_policy *, const float *in, size_t n, float *out, float init, int op);
ZS_ROCM_EXPORT void zs_rocm_reduce_f64(zs_rocm_policy *, const double *in, size_t n, double *out, double init, int op);
/* op: 0 = plus, 1 = multiplies, 2 = getmin, 3 = getmax (ZpcFunctional.hpp) */
ZS_ROCM_EXPORT void zs_rocm_scan_i32(zs_rocm_policy *, const int32_t *in, size_t n, int32_t *out, int32_t init, int op, int exclusive);
ZS_ROCM_EXPORT void zs_rocm_scan_i64(zs_rocm_policy *, const int64_t *in, size_t n, int64_t *out, int64_t init, int op, int exclusive);
ZS_ROCM_EXPORT void zs_rocm_scan_f32(zs_rocm_policy *, const float *in, size_t n, float *out, float init, int op, int exclusive);
ZS_ROCM_EXPORT void zs_rocm_scan_f64(zs_rocm_policy *, const double *in, size_t n, double *out, double init, int op, int exclusive);
/* stable radix sort on bits [sbit, ebit) of the sign-flipped key -- the order of zs::radix_sort / radix_sort_pair
 * (execution/ExecutionPolicy.hpp:765-781; cuda: cub::DeviceRadixSort, cuda/execution/ExecutionPolicy.cuh:755-881); vals may be NULL for
 * keys-only; kout may alias kin (the reference stages through temporaries).  Temporaries come from the policy's stream arena.
 * Up to 2 048 000 4-byte keys in contiguous arrays take three launches (top-digit split + buckets finished in LDS), everything else
 * one onesweep pass per 8 bits; the result is the same stable order either way. */
ZS_ROCM_EXPORT void zs_rocm_radix_sort_i32(zs_rocm_policy *, const int32_t *kin, const int32_t *vin, int32_t *kout, int32_t *vout, size_t n, int sbit, int ebit);
ZS_ROCM_EXPORT void zs_rocm_radix_sort_u32(zs_rocm_policy *, const uint32_t *kin, const int32_t *vin, uint32_t *kout, int32_t *vout, size_t n, int sbit, int ebit);
ZS_ROCM_EXPORT void zs_rocm_radix_sort_i64(zs_rocm_policy *, const int64_t *kin, const int32_t *vin, int64_t *kout, int32_t *vout, size_t n, int sbit, int ebit);
ZS_ROCM_EXPORT void zs_rocm_radix_sort_u64(zs_rocm_policy *, const uint64_t *kin, const int32_t *vin, uint64_t *kout, int32_t *vout, size_t n, int sbit, int ebit);
/* stable in-place merge sort (zs::merge_sort / merge_sort_pair, execution/ExecutionPolicy.hpp:745-761,
 * cuda/execution/ExecutionPolicy.cuh:698-752); `descending` != 0 sorts with `>`; vals may be NULL for keys-only.
 * User comparators: include/zensim_rocm/merge_sort.hpp through the C++ face. */
ZS_ROCM_EXPORT void zs_rocm_merge_sort_i32(zs_rocm_policy *, int32_t *keys, int32_t *vals, size_t n, int descending);
ZS_ROCM_EXPORT void zs_rocm_merge_sort_u32(zs_rocm_policy *, uint32_t *keys, int32_t *vals, size_t n, int descending);
ZS_ROCM_EXPORT void zs_rocm_merge_sort_i64(zs_rocm_policy *, int64_t *keys, int32_t *vals, size_t n, int descending);
ZS_ROCM_EXPORT void zs_rocm_merge_sort_u64(zs_rocm_policy *, uint64_t *keys, int32_t *vals, size_t n, int descending);
ZS_ROCM_EXPORT void zs_rocm_merge_sort_f32(zs_rocm_policy *, float *keys, int32_t *vals, size_t n, int descending);
ZS_ROCM_EXPORT void zs_rocm_merge_sort_f64(zs_rocm_policy *, double *keys, int32_t *vals, size_t n, int descending);

/* ======================================================================== (A) allocators & Vector */
/* py_interop/Allocator.cpp:5-21; memsrc_e: 0 = host, 1 = device, 2 = um (types/Property.h:7).
 * allocator_virtual = ZSPmrAllocator<true> over get_virtual_memory_source(mre, devid, reservedSpace, "STACK"): containers
 * created with it reserve `reservedSpace` bytes of address space (hipMemAddressReserve) and map physical memory as they
 * grow (hipMemCreate / hipMemMap), so their data pointer survives resize.  Every container entry point below also
 * exists with the reference's `_virtual` suffix; both spellings accept the same handle types. */
typedef struct zs_rocm_allocator zs_rocm_allocator;
ZS_ROCM_EXPORT zs_rocm_allocator *allocator(int memsrc, int8_t devid);
ZS_ROCM_EXPORT zs_rocm_allocator *allocator_virtual(int memsrc, int8_t devid, size_t reservedSpace);
ZS_ROCM_EXPORT void del_allocator(zs_rocm_allocator *);
ZS_ROCM_EXPORT void del_allocator_virtual(zs_rocm_allocator *);
ZS_ROCM_EXPORT int mem_enum__host(void);
ZS_ROCM_EXPORT int mem_enum__device(void);
ZS_ROCM_EXPORT int mem_enum__um(void);

/* py_interop/VectorInstantiations.cpp:8-170: zs::Vector<T> (container/Vector.hpp:11-421) */
typedef struct { void *_vector; } zs_rocm_vector_view_lite; /* VectorViewLite<T>, py_interop/VectorView.hpp:6-30 */
#define ZS_ROCM_DECL_VECTOR(T, SFX)                                                                       \
  ZS_ROCM_EXPORT zs_rocm_vector_##T *container__v_##T##SFX(zs_rocm_allocator *, size_t n);                \
  ZS_ROCM_EXPORT void del_container__v_##T##SFX(zs_rocm_vector_##T *);                                    \
  ZS_ROCM_EXPORT void relocate_container__v_##T##SFX(zs_rocm_vector_##T *, int memsrc, int8_t devid);     \
  ZS_ROCM_EXPORT void resize_container__v_##T##SFX(zs_rocm_vector_##T *, size_t n);                       \
  ZS_ROCM_EXPORT void reset_container__v_##T##SFX(zs_rocm_vector_##T *, int byteVal);                     \
  ZS_ROCM_EXPORT size_t container_size__v_##T##SFX(const zs_rocm_vector_##T *);                           \
  ZS_ROCM_EXPORT size_t container_capacity__v_##T##SFX(const zs_rocm_vector_##T *);                       \
  ZS_ROCM_EXPORT T get_val_container__v_##T##SFX(zs_rocm_vector_##T *);            /* getVal()      */   \
  ZS_ROCM_EXPORT void set_val_container__v_##T##SFX(zs_rocm_vector_##T *, T v);    /* setVal(v)     */   \
  ZS_ROCM_EXPORT T get_val_i_container__v_##T##SFX(zs_rocm_vector_##T *, size_t i);                       \
  ZS_ROCM_EXPORT void set_val_i_container__v_##T##SFX(zs_rocm_vector_##T *, size_t i, T v);              \
  ZS_ROCM_EXPORT void copy_to_container__v_##T##SFX(zs_rocm_vector_##T *, void *hostSrc);   /* assignVals   */ \
  ZS_ROCM_EXPORT void copy_from_container__v_##T##SFX(zs_rocm_vector_##T *, void *hostDst); /* retrieveVals */ \
  ZS_ROCM_EXPORT T *get_handle_container__v_##T##SFX(zs_rocm_vector_##T *);                               \
  ZS_ROCM_EXPORT zs_rocm_vector_view_lite *pyview__v_##T##SFX(zs_rocm_vector_##T *);                      \
  ZS_ROCM_EXPORT zs_rocm_vector_view_lite *pyview__v_const_##T##SFX(const zs_rocm_vector_##T *);          \
  ZS_ROCM_EXPORT aosoa_iterator_##T##_1 get_iterator_1__v_##T##SFX(zs_rocm_vector_##T *, uint32_t id);    \
  ZS_ROCM_EXPORT aosoa_iterator_const_##T##_1 get_iterator_1__v_const_##T##SFX(const zs_rocm_vector_##T *, uint32_t id); \
  ZS_ROCM_EXPORT aosoa_iterator_##T##_3 get_iterator_3__v_##T##SFX(zs_rocm_vector_##T *, uint32_t id);    \
  ZS_ROCM_EXPORT aosoa_iterator_const_##T##_3 get_iterator_3__v_const_##T##SFX(const zs_rocm_vector_##T *, uint32_t id);
#define ZS_ROCM_DECL_VECTOR_BOTH(T)                                                    \
  typedef struct zs_rocm_vector_##T zs_rocm_vector_##T;                                \
  ZS_ROCM_DECL_VECTOR(T, )                                                             \
  ZS_ROCM_DECL_VECTOR(T, _virtual)                                                     \
  ZS_ROCM_EXPORT void del_pyview__v_##T(zs_rocm_vector_view_lite *);                   \
  ZS_ROCM_EXPORT void del_pyview__v_const_##T(zs_rocm_vector_view_lite *);             \
  ZS_ROCM_EXPORT T *container_data__v_##T(zs_rocm_vector_##T *);
ZS_ROCM_DECL_VECTOR_BOTH(int)
ZS_ROCM_DECL_VECTOR_BOTH(float)
ZS_ROCM_DECL_VECTOR_BOTH(double)

/* ======================================================================== (A) TileVector */
/* py_interop/TileVectorInstantiations.cpp:8-215: property tags + zs::TileVector<T, L>
 * (container/TileVector.hpp:14-561).  Storage: element (chn, i) at (i/L*C + chn)*L + i%L. */
typedef struct zs_rocm_property_tags zs_rocm_property_tags;
ZS_ROCM_EXPORT zs_rocm_property_tags *property_tags(const char *const *names, const int *sizes, size_t n);
ZS_ROCM_EXPORT void del_property_tags(zs_rocm_property_tags *);
ZS_ROCM_EXPORT void property_tags_get_item(zs_rocm_property_tags *, size_t index, const char **name, size_t *size);
ZS_ROCM_EXPORT size_t property_tags_get_size(zs_rocm_property_tags *);
typedef struct {
  void *_vector;
  int _numChannels;
} zs_rocm_tv_view_lite; /* TileVectorViewLite<T, L>, py_interop/TileVectorView.hpp:9-131 */
typedef struct {
  void *_vector;
  int _numChannels;
  const char *_tagNames; /* [N] SmallString = char[32], in the container's memory space (TileVector.hpp:503-509) */
  const int *_tagOffsets;
  const int *_tagSizes;
  int _N;
} zs_rocm_tv_named_view_lite; /* TileVectorNamedViewLite<T, L>, py_interop/TileVectorView.hpp:133-287 */
#define ZS_ROCM_DECL_TILEVECTOR(T, L, SFX)                                                                      \
  ZS_ROCM_EXPORT zs_rocm_tv_##T##_##L *container__tv_##T##_##L##SFX(zs_rocm_allocator *,                        \
                                                                   const zs_rocm_property_tags *, size_t n);   \
  ZS_ROCM_EXPORT void del_container__tv_##T##_##L##SFX(zs_rocm_tv_##T##_##L *);                                 \
  ZS_ROCM_EXPORT void relocate_container__tv_##T##_##L##SFX(zs_rocm_tv_##T##_##L *, int memsrc, int8_t devid);  \
  ZS_ROCM_EXPORT void resize_container__tv_##T##_##L##SFX(zs_rocm_tv_##T##_##L *, size_t n);                    \
  ZS_ROCM_EXPORT void reset_container__tv_##T##_##L##SFX(zs_rocm_tv_##T##_##L *, int byteVal);                  \
  ZS_ROCM_EXPORT size_t container_size__tv_##T##_##L##SFX(const zs_rocm_tv_##T##_##L *);                        \
  ZS_ROCM_EXPORT size_t container_capacity__tv_##T##_##L##SFX(const zs_rocm_tv_##T##_##L *);                    \
  ZS_ROCM_EXPORT int property_offset__tv_##T##_##L##SFX(const zs_rocm_tv_##T##_##L *, const char *name);        \
  ZS_ROCM_EXPORT int property_size__tv_##T##_##L##SFX(const zs_rocm_tv_##T##_##L *, const char *name);          \
  ZS_ROCM_EXPORT aosoa_iterator_##T##_1 get_iterator_1__tv_##T##_##L##SFX(zs_rocm_tv_##T##_##L *, uint32_t id,  \
                                                                          uint32_t chnOffset);                 \
  ZS_ROCM_EXPORT aosoa_iterator_const_##T##_1 get_iterator_1__tv_const_##T##_##L##SFX(const zs_rocm_tv_##T##_##L *, \
                                                                                      uint32_t id, uint32_t chnOffset); \
  ZS_ROCM_EXPORT aosoa_iterator_##T##_3 get_iterator_3__tv_##T##_##L##SFX(zs_rocm_tv_##T##_##L *, uint32_t id,  \
                                                                          uint32_t chnOffset);                 \
  ZS_ROCM_EXPORT aosoa_iterator_const_##T##_3 get_iterator_3__tv_const_##T##_##L##SFX(const zs_rocm_tv_##T##_##L *, \
                                                                                      uint32_t id, uint32_t chnOffset); \
  ZS_ROCM_EXPORT zs_rocm_tv_view_lite *pyview__tv_##T##_##L##SFX(zs_rocm_tv_##T##_##L *);                       \
  ZS_ROCM_EXPORT zs_rocm_tv_view_lite *pyview__tv_const_##T##_##L##SFX(const zs_rocm_tv_##T##_##L *);           \
  ZS_ROCM_EXPORT zs_rocm_tv_named_view_lite *pyview__tvn_##T##_##L##SFX(zs_rocm_tv_##T##_##L *);                \
  ZS_ROCM_EXPORT zs_rocm_tv_named_view_lite *pyview__tvn_const_##T##_##L##SFX(const zs_rocm_tv_##T##_##L *);    \
  /* py_interop/cuda/TileVectorUtility.cpp:7-30 -> append_channels (TileVector.hpp:583-623) */                 \
  ZS_ROCM_EXPORT void append_properties__rocm_tv_##T##_##L##SFX(zs_rocm_policy *, zs_rocm_tv_##T##_##L *,       \
                                                               const zs_rocm_property_tags *);
#define ZS_ROCM_DECL_TILEVECTOR_BOTH(T, L)                                                                 \
  typedef struct zs_rocm_tv_##T##_##L zs_rocm_tv_##T##_##L;                                                \
  ZS_ROCM_DECL_TILEVECTOR(T, L, )                                                                          \
  ZS_ROCM_DECL_TILEVECTOR(T, L, _virtual)                                                                  \
  ZS_ROCM_EXPORT void del_pyview__tv_##T##_##L(zs_rocm_tv_view_lite *);                                    \
  ZS_ROCM_EXPORT void del_pyview__tv_const_##T##_##L(zs_rocm_tv_view_lite *);                              \
  ZS_ROCM_EXPORT void del_pyview__tvn_##T##_##L(zs_rocm_tv_named_view_lite *);                             \
  ZS_ROCM_EXPORT void del_pyview__tvn_const_##T##_##L(zs_rocm_tv_named_view_lite *);                       \
  ZS_ROCM_EXPORT size_t container_num_channels__tv_##T##_##L(const zs_rocm_tv_##T##_##L *);                \
  ZS_ROCM_EXPORT T *container_data__tv_##T##_##L(zs_rocm_tv_##T##_##L *);                                  \
  /* (B) TileVector::reset(pol, val) TileVector.hpp:624-640 */                                            \
  ZS_ROCM_EXPORT void zs_rocm_fill__tv_##T##_##L(zs_rocm_policy *, zs_rocm_tv_##T##_##L *, T val);         \
  /* (B) TileVector::reorderTiles-style element reorder (TileVector.hpp:641-691): dst(:, i) = src(:, map[i]) \
     when gather != 0, dst(:, map[i]) = src(:, i) otherwise; all channels */                              \
  ZS_ROCM_EXPORT void zs_rocm_reorder__tv_##T##_##L(zs_rocm_policy *, zs_rocm_tv_##T##_##L *,              \
                                                   const int *map, int gather);
ZS_ROCM_DECL_TILEVECTOR_BOTH(int, 8)
ZS_ROCM_DECL_TILEVECTOR_BOTH(int, 32)
ZS_ROCM_DECL_TILEVECTOR_BOTH(int, 64)
ZS_ROCM_DECL_TILEVECTOR_BOTH(int, 512)
ZS_ROCM_DECL_TILEVECTOR_BOTH(float, 8)
ZS_ROCM_DECL_TILEVECTOR_BOTH(float, 32)
ZS_ROCM_DECL_TILEVECTOR_BOTH(float, 64)
ZS_ROCM_DECL_TILEVECTOR_BOTH(float, 512)
ZS_ROCM_DECL_TILEVECTOR_BOTH(double, 8)
ZS_ROCM_DECL_TILEVECTOR_BOTH(double, 32)
ZS_ROCM_DECL_TILEVECTOR_BOTH(double, 64)
ZS_ROCM_DECL_TILEVECTOR_BOTH(double, 512)

/* (B) raw AoSoA kernels on plain device pointers (what `pol(range(n), [tv = view<space>(tv)](i){...})`
 * load/store lambdas do, test/cuda/basic.cu:118-144).  tv has C channels of tile width L (power of 2). */
ZS_ROCM_EXPORT void zs_rocm_tv_from_aos_f32(zs_rocm_policy *, const float *aos, size_t n, int C, int L, float *tv);
ZS_ROCM_EXPORT void zs_rocm_tv_to_aos_f32(zs_rocm_policy *, const float *tv, size_t n, int C, int L, float *aos);
/* load every channel, scale by `alpha`, store back (BASELINE config 2 "AoSoA load/store": 8*C bytes/element) */
ZS_ROCM_EXPORT void zs_rocm_tv_scale_f32(zs_rocm_policy *, float *tv, size_t n, int C, int L, float alpha);
/* rows map[j] of an AoSoA buffer -> AoS rows j, and AoS rows j -> elements dstOffset + j of an AoSoA buffer: the pack / unpack
 * of the inter-rank particle migration ("ncclSend/Recv of AoSoA tiles after a per-destination radix partition") */
ZS_ROCM_EXPORT void zs_rocm_tv_gather_rows_f32(zs_rocm_policy *, const float *tv, const int *map, size_t m, int C, int L, float *aos);
ZS_ROCM_EXPORT void zs_rocm_tv_scatter_rows_f32(zs_rocm_policy *, const float *aos, size_t m, int C, int L, float *tv, size_t dstOffset);
ZS_ROCM_EXPORT void zs_rocm_tv_gather_f32(zs_rocm_policy *, const float *src, float *dst, size_t n, int C, int L, const int *map);
/* the same for the channels whose bit is set in channelMask only (C <= 64); the other channels of dst are left untouched */
ZS_ROCM_EXPORT void zs_rocm_tv_gather_channels_f32(zs_rocm_policy *, const float *src, float *dst, size_t n, int C, int L, const int *map,
                                                   unsigned long long channelMask);

/* ======================================================================== (A) bht */
/* py_interop/BhtInstantiations.cpp:6-128: zs::bht<int, dim, int, B>, dim 1-4, B = 16 | 32 (container/Bht.hpp:16-272).
 * Table layout identical to the reference: keys [tableSize] of next_2pow(dim) ints (unused/padding
 * ints hold 0x3f3f3f3f), indices [tableSize], status [tableSize] (all -1 outside of a build),
 * activeKeys [tableSize][dim], cnt, buildSuccess; tableSize = evaluateTableSize(n) (Bht.hpp:154-158);
 * hash functions seeded from std::mt19937(2) (Bht.hpp:165-169). */
typedef struct {
  void *keys;       /* storage_key_type* */
  int *indices;
  int *status;
  void *activeKeys; /* key_type* */
  int *cnt;
  int *success;
  uint32_t tableSize, numBuckets; /* size_type = u32 (BhtView.hpp:13); numBuckets = tableSize / B (:107) */
  uint32_t hf0x, hf0y, hf1x, hf1y, hf2x, hf2y;
} zs_rocm_bht_view_lite; /* BhtViewLite members, py_interop/BhtView.hpp:1054-1062; byte layout checked against
                            tests/golden/abi_layout.json (derived from the reference headers by tools/gen_abi_layout.sh) */
#define ZS_ROCM_DECL_BHT_A(D, B, SFX)                                                                         \
  ZS_ROCM_EXPORT zs_rocm_bht_##D *container__bht_int_##D##_int_##B##SFX(zs_rocm_allocator *, size_t n);        \
  ZS_ROCM_EXPORT void del_container__bht_int_##D##_int_##B##SFX(zs_rocm_bht_##D *);                            \
  ZS_ROCM_EXPORT void relocate_container__bht_int_##D##_int_##B##SFX(zs_rocm_bht_##D *, int memsrc, int8_t devid); \
  ZS_ROCM_EXPORT size_t container_size__bht_int_##D##_int_##B##SFX(const zs_rocm_bht_##D *);                   \
  ZS_ROCM_EXPORT size_t container_capacity__bht_int_##D##_int_##B##SFX(const zs_rocm_bht_##D *);               \
  ZS_ROCM_EXPORT void reset_container__bht_int_##D##_int_##B##SFX(zs_rocm_bht_##D *, int clearCnt);            \
  ZS_ROCM_EXPORT zs_rocm_bht_view_lite *pyview__bht_int_##D##_int_##B##SFX(zs_rocm_bht_##D *);                 \
  ZS_ROCM_EXPORT zs_rocm_bht_view_lite *pyview__bht_const_int_##D##_int_##B##SFX(const zs_rocm_bht_##D *);     \
  /* py_interop/cuda/BhtUtility.cpp:7-26 -> bht::resize (Bht.hpp:320-340) */                                  \
  ZS_ROCM_EXPORT void resize_container__rocm_bht_int_##D##_int_##B##SFX(zs_rocm_policy *, zs_rocm_bht_##D *,   \
                                                                       size_t newCapacity);
#define ZS_ROCM_DECL_BHT(D, B)                                                                           \
  ZS_ROCM_DECL_BHT_A(D, B, )                                                                             \
  ZS_ROCM_DECL_BHT_A(D, B, _virtual)                                                                     \
  ZS_ROCM_EXPORT void del_pyview__bht_int_##D##_int_##B(zs_rocm_bht_view_lite *);                         \
  /* (B) pol(range(n), [tb](i){ ret[i] = tb.insert(keys[i]); })  BHTView::insert, Bht.hpp:490-542 */     \
  ZS_ROCM_EXPORT void zs_rocm_insert__bht_int_##D##_int_##B(zs_rocm_policy *, zs_rocm_bht_##D *,          \
                                                          const int *keys, size_t n, int *ret);         \
  /* (B) table := { keys[i] -> index i }, cnt = n: adopt a partition numbered elsewhere (e.g. the _activeKeys of a  \
     zs::HashTable, container/HashTable.hpp, which the reference's in-tree P2G/G2P use); insert(key, i, enqueue)   \
     of Bht.hpp:490-542 with a fixed index */                                                                     \
  ZS_ROCM_EXPORT void zs_rocm_assign__bht_int_##D##_int_##B(zs_rocm_policy *, zs_rocm_bht_##D *,          \
                                                          const int *keys, size_t n);                   \
  /* (B) pol(range(n), [tb](i){ ret[i] = tb.query(keys[i]); })  BHTView::query, Bht.hpp:667-698 */       \
  ZS_ROCM_EXPORT void zs_rocm_query__bht_int_##D##_int_##B(zs_rocm_policy *, const zs_rocm_bht_##D *,     \
                                                         const int *keys, size_t n, int *ret);          \
  /* (B) bht::reorder(pol, map, scatter|gather), Bht.hpp:377-400 */                                      \
  ZS_ROCM_EXPORT void zs_rocm_reorder__bht_int_##D##_int_##B(zs_rocm_policy *, zs_rocm_bht_##D *,         \
                                                           const int *map, int scatter);                \
  /* (B) canonical form for bit-exact comparison (SURVEY.md 8a note): sort active keys               \
     lexicographically and renumber */                                                                  \
  ZS_ROCM_EXPORT void zs_rocm_canonicalize__bht_int_##D##_int_##B(zs_rocm_policy *, zs_rocm_bht_##D *);  \
  /* ... with the significance of the key's components chosen: axes = a permutation of 0 .. D-1 (host array), axes[0] \
     the most significant component, axes[D-1] the one that changes fastest along the numbering; NULL = 0, 1, ..       \
     Returns 0, -1 if axes is not a permutation */                                                                     \
  ZS_ROCM_EXPORT int zs_rocm_canonicalize_axes__bht_int_##D##_int_##B(zs_rocm_policy *, zs_rocm_bht_##D *, const int *axes);  \
  /* ... and only the entries [first, size): the head keeps its numbers (an MPM partition: the blocks that hold particles, numbered \
     before EnlargeSparsity appended the apron blocks -- sorting the tail makes the whole numbering reproducible) */              \
  ZS_ROCM_EXPORT int zs_rocm_canonicalize_tail__bht_int_##D##_int_##B(zs_rocm_policy *, zs_rocm_bht_##D *, const int *axes,     \
                                                                     size_t first);                                             \
  /* (B) renumber the active keys along the Z-order (Morton) curve of (key - min key): consecutive  \
     entries are spatial neighbours -- the launch order the per-block MPM kernels want (no reference  \
     counterpart: the reference's numbering is insertion order, Bht.hpp:612-664, and any numbering is \
     a valid table) */                                                                                  \
  ZS_ROCM_EXPORT void zs_rocm_order_morton__bht_int_##D##_int_##B(zs_rocm_policy *, zs_rocm_bht_##D *);
typedef struct zs_rocm_bht_1 zs_rocm_bht_1; /* one handle type per dim; the bucket size is a field of the object */
typedef struct zs_rocm_bht_2 zs_rocm_bht_2;
typedef struct zs_rocm_bht_3 zs_rocm_bht_3;
typedef struct zs_rocm_bht_4 zs_rocm_bht_4;
ZS_ROCM_DECL_BHT(1, 16)
ZS_ROCM_DECL_BHT(2, 16)
ZS_ROCM_DECL_BHT(3, 16)
ZS_ROCM_DECL_BHT(4, 16)
ZS_ROCM_DECL_BHT(1, 32)
ZS_ROCM_DECL_BHT(2, 32)
ZS_ROCM_DECL_BHT(3, 32)
ZS_ROCM_DECL_BHT(4, 32)

/* ======================================================================== (B) HashTable */
/* zs::HashTable<i32, dim, int> (container/HashTable.hpp:16-592), dim 1-4: the open-addressing table (64-bit hash_combine
 * chain over the raw coordinates `:496-500`, home = ((h % size) + size) % size, linear probing with stride 127 `:362`)
 * that `partition_for_particles` returns (simulation/sparsity/SparsityCompute.tpp:5-24) and the Grids-based MPM path keys
 * its blocks with (simulation/mpm/Simulator.cpp:122).  The reference exposes it only as a C++ template; these entry
 * points are the bulk forms of `pol(range(n), [t = proxy<space>(table)](i){ ... t.insert(key_i) ... })`.
 * Layout as in the reference: keys [tableSize][dim] packed ints (empty = INT_MAX), indices (-1 = empty), status (-1),
 * activeKeys [tableSize][dim], cnt; tableSize = next_2pow(n) * 16 (`:87-90`). */
typedef struct zs_rocm_hashtable zs_rocm_hashtable;
typedef struct {
  int *keys, *indices, *status, *activeKeys, *cnt;
  int tableSize;
} zs_rocm_hashtable_view; /* HashTableView members, HashTable.hpp:472-476 */
ZS_ROCM_EXPORT zs_rocm_hashtable *zs_rocm_hashtable_create(int dim, size_t numExpectedEntries, int memsrc, int devid);
ZS_ROCM_EXPORT void zs_rocm_hashtable_destroy(zs_rocm_hashtable *);
ZS_ROCM_EXPORT int zs_rocm_hashtable_dim(const zs_rocm_hashtable *);
ZS_ROCM_EXPORT size_t zs_rocm_hashtable_table_size(const zs_rocm_hashtable *); /* _tableSize */
ZS_ROCM_EXPORT int zs_rocm_hashtable_size(const zs_rocm_hashtable *);          /* size(): device -> host copy of cnt (:152) */
ZS_ROCM_EXPORT void zs_rocm_hashtable_get_view(const zs_rocm_hashtable *, zs_rocm_hashtable_view *out);
/* HashTable::reset(pol, clearCnt) (:294-299) == CleanSparsity with clearCnt = 1 (sparsity/SparsityOp.hpp:42-57) */
ZS_ROCM_EXPORT void zs_rocm_hashtable_reset(zs_rocm_policy *, zs_rocm_hashtable *, int clearCnt);
/* HashTableView::insert(key) (:353-374): ret[i] = dense index for the one inserter of a new key, -1 (sentinel_v) otherwise */
ZS_ROCM_EXPORT void zs_rocm_hashtable_insert(zs_rocm_policy *, zs_rocm_hashtable *, const int *keys, size_t n, int *ret);
/* HashTableView::insert(key, id) (:405-421): indices[slot] = ids[i] (ids == NULL: i); ok[i] = 1 if this call created the entry */
ZS_ROCM_EXPORT void zs_rocm_hashtable_insert_ids(zs_rocm_policy *, zs_rocm_hashtable *, const int *keys, const int *ids, size_t n, int *ok);
/* HashTableView::query / entry (:445-470): index / slot of a key, -1 if absent (table quiescent) */
ZS_ROCM_EXPORT void zs_rocm_hashtable_query(zs_rocm_policy *, const zs_rocm_hashtable *, const int *keys, size_t n, int *ret);
ZS_ROCM_EXPORT void zs_rocm_hashtable_entry(zs_rocm_policy *, const zs_rocm_hashtable *, const int *keys, size_t n, int *ret);
/* HashTable::resize / preserve (:258-292) */
ZS_ROCM_EXPORT void zs_rocm_hashtable_resize(zs_rocm_policy *, zs_rocm_hashtable *, size_t numExpectedEntries);
ZS_ROCM_EXPORT void zs_rocm_hashtable_preserve(zs_rocm_policy *, zs_rocm_hashtable *, size_t numExpectedEntries);

/* ======================================================================== (B) LBvh */
/* zs::LBvh<3, int, f32> (container/Bvh.hpp:86-492): linear BVH over AABBs, Karras (2012) topology on sorted 30-bit morton
 * codes, stored in depth-first pre-order with escape indices for stack-less traversal.  Boxes are AABBBox<3, f32> =
 * [n][6] floats {min xyz, max xyz} in device memory.  The reference exposes it only as a C++ template
 * (`bvh.build(pol, primBvs)`, `pol(range(n), [bvh = proxy<space>(bvh)](i){ bvh.iter_neighbors(bv, f); })`). */
typedef struct zs_rocm_lbvh zs_rocm_lbvh;
typedef struct {
  float *orderedBvs; /* [numNodes][6] */
  int *parents, *levels, *leafInds, *auxIndices;
  int numNodes, numLeaves;
} zs_rocm_lbvh_view; /* LBvhView members, Bvh.hpp:790-792 */
ZS_ROCM_EXPORT zs_rocm_lbvh *zs_rocm_lbvh_create(void);
ZS_ROCM_EXPORT void zs_rocm_lbvh_destroy(zs_rocm_lbvh *);
ZS_ROCM_EXPORT size_t zs_rocm_lbvh_num_leaves(const zs_rocm_lbvh *); /* getNumLeaves, :125 */
ZS_ROCM_EXPORT size_t zs_rocm_lbvh_num_nodes(const zs_rocm_lbvh *);  /* getNumNodes, :126-129: 2n-1, or n when n <= 2 */
ZS_ROCM_EXPORT void zs_rocm_lbvh_get_view(const zs_rocm_lbvh *, zs_rocm_lbvh_view *out);
/* LBvh::build(pol, primBvs, wrapv<Refit>) (:810-1082); n == 0 is a no-op, n <= 2 stores the boxes themselves */
ZS_ROCM_EXPORT void zs_rocm_lbvh_build(zs_rocm_policy *, zs_rocm_lbvh *, const float *primBvs, size_t n, int refit);
/* LBvh::refit (:1219-1248); returns -1 (the reference throws) when n differs from the built leaf count */
ZS_ROCM_EXPORT int zs_rocm_lbvh_refit(zs_rocm_policy *, zs_rocm_lbvh *, const float *primBvs, size_t n);
/* LBvh::getTotalBox (:152-171) -> box6 (device pointer, 6 floats) */
ZS_ROCM_EXPORT void zs_rocm_lbvh_total_box(zs_rocm_policy *, const zs_rocm_lbvh *, float *box6);
/* bulk LBvhView::iter_neighbors (:644-680): counts[q] = number of primitives whose box overlaps queryBvs[q]; then, with
 * offsets = exclusive_scan(counts), out[offsets[q] ...] = their ids in traversal order */
/* (r04: 16384 or more queries are walked in Morton order of their centres -- codes + one pair sort inside the call; every query's
 * result still goes to its own slot, hits in the walk's order) */
ZS_ROCM_EXPORT void zs_rocm_lbvh_query_count(zs_rocm_policy *, const zs_rocm_lbvh *, const float *queryBvs, size_t nq, int *counts);
ZS_ROCM_EXPORT void zs_rocm_lbvh_query_fill(zs_rocm_policy *, const zs_rocm_lbvh *, const float *queryBvs, size_t nq, const int *offsets,
                                            int *out);
/* self-collision broadphase (LBvhView::self_iter_neighbors, container/Bvh.hpp:695-728, driven over every leaf): thread k walks
 * from the k-th leaf in node order; counts[k] = overlapping leaves AFTER it (the leaf itself is skipped), so every unordered
 * pair of overlapping primitives appears exactly once.  fill: pairs[2*(offsets[k]+c)] = {primitive of leaf k, other primitive}.
 * The count pass remembers the first 32 hits of every leaf inside the LBvh object (132 B per leaf: 1.3 GB for 10 M leaves, allocated on
 * the first self query); a fill pass on the unchanged tree copies them instead of walking again (the memory is released with the
 * object, invalidated by build / refit).  `pairs` must be 8-byte aligned (any hipMalloc'ed array is).  `offsets` may be any per-leaf start
 * (the exclusive scan of `counts` is the fast case: a wave then writes its leaves' runs as one contiguous stream).  r04: one walk per WAVE over the
 * union of its 64 leaves' walks; every leaf still reports the same ids in the same order. */
ZS_ROCM_EXPORT void zs_rocm_lbvh_self_query_count(zs_rocm_policy *, const zs_rocm_lbvh *, int *counts /* [numLeaves] */);
ZS_ROCM_EXPORT void zs_rocm_lbvh_self_query_fill(zs_rocm_policy *, const zs_rocm_lbvh *, const int *offsets, int *pairs);

/* ======================================================================== (B) MPM transfers */
/* A particle attribute stored in an AoS zs::Vector<vec<T,N>> (geometry/Structurefree.hpp:21-237) or in
 * a TileVector channel group: component d of particle i lives at
 *   base + ((((i >> numTileBits) * numChns) << numTileBits) | (i & tileMask)) + d * (tileMask + 1)
 * (py_interop/GenericIterator.hpp:95-101). */
typedef aosoa_iterator_float_1 zs_rocm_attr;

typedef struct {
  zs_rocm_attr mass;  /* 1 */
  zs_rocm_attr pos;   /* 3 */
  zs_rocm_attr vel;   /* 3 */
  zs_rocm_attr C;     /* 9, column-major */
  zs_rocm_attr F;     /* 9, column-major */
  zs_rocm_attr logJp; /* 1, plastic models only (base may be NULL otherwise) */
  zs_rocm_attr stress; /* 6 = {xx, xy, xz, yy, yz, zz} of the symmetric P F^T * volume (the Kirchhoff stress times the volume:
                          symmetric for every isotropic model of P2G.hpp:82-101; r04, was 9), optional (base NULL = off): the
                          cached result of the constitutive update.  When present,
                          zs_rocm_mpm_g2p evaluates the model on the F it has just updated (and updates logJp) and stores the
                          result here, and zs_rocm_mpm_p2g reads it instead of re-running the 3x3 SVD: the per-particle
                          constitutive work of the reference's P2G (P2G.hpp:60-101) moves to the tail of the previous G2P, where
                          the VALU is idle.  Call zs_rocm_mpm_update_stress once before the first P2G and after any host-side
                          edit of F / logJp. */
  size_t n;
} zs_rocm_particles;

enum {
  ZS_MPM_FIXED_COROTATED = 0, ZS_MPM_DRUCKER_PRAGER = 1, ZS_MPM_VONMISES_FIXED_COROTATED = 2, ZS_MPM_NACC = 3,
  /* EquationOfStateConfig (weakly compressible fluid): the particles carry the volume ratio J instead of F -- pass the
   * 1-channel `J` attribute as zs_rocm_particles::F (only component 0 is read / written: G2P does J <- (1 + tr(C) dt) J,
   * simulation/transfer/G2P.hpp:70-74; P2G.hpp:60-81 forms the stress from J and C) */
  ZS_MPM_EQUATION_OF_STATE = 4
};
typedef struct {
  int model;          /* FixedCorotatedConfig | DruckerPragerConfig (physics/ConstitutiveModel.hpp:739-757) */
  float dx, dt;
  float volume, E, nu;
  float cohesion, beta, yieldSurface;
  int volCorrection;
  int side;           /* grid block side: 4 = Grids<f32,3,4> (geometry/Structure.hpp), 8 = SparseGrid<3,f32,8> */
  int keyIsOrigin;    /* 0: partition keys are block coordinates cell/side (Grids + HashTable/bht, simulation/Utils.hpp:24-31);
                         1: keys are block origins in cells, multiples of side (SparseGrid, geometry/SparseGrid.hpp:305-309) */
  float yieldStress;  /* VonMisesFixedCorotatedConfig::yieldStress (physics/ConstitutiveModel.hpp:745-749) */
  float xi, Msqr;     /* NACCConfig::xi, NACCConfig::Msqr() (:759-785; zs_rocm_nacc_msqr); NACC also uses E, nu, beta, logJp */
  int hardeningOn;    /* NACCConfig::hardeningOn */
  float bulk, viscosity; /* EquationOfStateConfig::bulk, ::viscosity (gamma is fixed to 7 by the formula, P2G.hpp:64-69) */
} zs_rocm_mpm_params;
/* NACCConfig::Msqr() for friction angle `fa` and dimension 3, evaluated as the reference does (physics/ConstitutiveModel.hpp:771-785) */
ZS_ROCM_EXPORT float zs_rocm_nacc_msqr(float fa);

/* grid: TileVector<f32, side^3> with 7 channels {m:1, v:3, rhs:3} (simulation/mpm/Simulator.cpp:116-122),
 * block b channel c cell k at grid[(b*7 + c)*side^3 + k], cell id = (x*side + y)*side + z
 * (geometry/Structure.hpp:323-333).  The partition is a bht<int,3,int,16> keyed by block coordinate
 * (cell coordinate / side), block number = table index. */

/* pol(range(n), ComputeSparsity{dx, side, table, X}) (sparsity/SparsityOp.hpp:59-87) */
ZS_ROCM_EXPORT void zs_rocm_mpm_compute_sparsity(zs_rocm_policy *, zs_rocm_bht_3 *, zs_rocm_attr pos, size_t n,
                                                 float dx, int side, int keyIsOrigin);
/* pol(range(nblocks), EnlargeSparsity{table, lo, hi}) (sparsity/SparsityOp.hpp:89-115) */
/* keyStride: 1 for block-coordinate keys, side for block-origin keys */
ZS_ROCM_EXPORT void zs_rocm_mpm_enlarge_sparsity(zs_rocm_policy *, zs_rocm_bht_3 *, const int lo[3], const int hi[3],
                                                 int keyStride);
/* ======================================================================== (B) IndexBuckets */
/* zs::IndexBuckets<3, i32, i32> (container/IndexBuckets.hpp:9-67) and `index_buckets_for_particles(pol, particles, dx,
 * displacement)` (simulation/particle/Query.tpp:9-58): a HashTable<i32,3,int> of occupied cells (key = floor(x/dx +
 * displacement), CleanSparsity + ComputeSparsity with blockLen 1, offset 0), counts[numBuckets+1] (SpatiallyCount,
 * simulation/sparsity/SparsityOp.hpp:117-152), offsets = exclusive_scan(counts), indices[n] = particle ids grouped by
 * bucket (SpatiallyDistribute, :154-196).  The reference fills a bucket in atomic race order; here ids are ascending
 * inside a bucket (= the sequential policy's result), so the structure is reproducible. */
typedef struct zs_rocm_index_buckets zs_rocm_index_buckets;
typedef struct {
  zs_rocm_hashtable *table; /* _table: bucket number = table.query(cell) */
  int *indices;             /* [numEntries] */
  int *offsets, *counts;    /* [numBuckets + 1] */
  int numBuckets, numEntries;
  float dx;
} zs_rocm_index_buckets_view; /* IndexBucketsView members, IndexBuckets.hpp:112-114 */
ZS_ROCM_EXPORT zs_rocm_index_buckets *zs_rocm_index_buckets_create(void);
ZS_ROCM_EXPORT void zs_rocm_index_buckets_destroy(zs_rocm_index_buckets *);
ZS_ROCM_EXPORT void zs_rocm_index_buckets_get_view(const zs_rocm_index_buckets *, zs_rocm_index_buckets_view *out);
/* `expectedCells` sizes the hash table (0: the particle count, as the reference does: tableSize = next_2pow(n) * 16) */
ZS_ROCM_EXPORT void zs_rocm_index_buckets_for_particles(zs_rocm_policy *, zs_rocm_index_buckets *, zs_rocm_attr pos, size_t n,
                                                        float dx, float displacement, size_t expectedCells);
/* Buckets over the cells of a block partition, for the gather-style transfers of a time loop: bucket number = block * side^3 + cell id
 * (the cell that contains the particle, displacement 0), counts / offsets / indices as above, but NO hash table is built (view.table ==
 * NULL, numBuckets = nblocks * side^3): zs_rocm_mpm_p2c2g finds a cell's bucket through the partition it is given anyway, which must be
 * this `table`.  Particles whose cell is not in the partition are listed in one extra bucket at index numBuckets that no transfer visits.
 * 4.4 -> 1.5 ms per rebuild at 16.7 M particles (no hash inserts). */
ZS_ROCM_EXPORT void zs_rocm_index_buckets_for_partition(zs_rocm_policy *, zs_rocm_index_buckets *, zs_rocm_attr pos, size_t n, float dx,
                                                        const zs_rocm_bht_3 *table, int side, int keyIsOrigin);
/* The same two functors on a zs::HashTable<i32,3,int> partition (their in-tree form: `partition_for_particles`,
 * simulation/sparsity/SparsityCompute.tpp:5-24 = CleanSparsity + ComputeSparsity(dx, blocklen, table, x), offset -2,
 * displacement 0.5; EnlargeSparsity sparsity/SparsityOp.hpp:89-115).  `zs_rocm_assign__bht_int_3_int_16(pol, bht,
 * view.activeKeys, size)` then adopts the block numbering for the binned transfers. */
ZS_ROCM_EXPORT void zs_rocm_mpm_partition_for_particles(zs_rocm_policy *, zs_rocm_hashtable *, zs_rocm_attr pos, size_t n,
                                                        float dx, int blocklen);
ZS_ROCM_EXPORT void zs_rocm_mpm_enlarge_sparsity__hashtable(zs_rocm_policy *, zs_rocm_hashtable *, const int lo[3],
                                                            const int hi[3]);

/* particle -> bin binning (the role of IndexBuckets / SpatiallyCount+Distribute,
 * sparsity/SparsityOp.hpp:117-196, simulation/particle/Query.tpp:9-58).  A bin is a 4x4x4 group of cells
 * (side 4: bin == grid block b; side 8: bin = 8*b + sub-cube).  Output: `order` [n], a permutation listing for
 * every bin, in [binStart[k], binStart[k+1]), the particles whose base node floor(x/dx - 0.5) lies in bin k,
 * round-robin over the bin's 64 cells (round r = the r-th particle of every cell that has one, cells in
 * x-major order); `cellCount` [nbins*64] particles per cell; binStart [nbins+1].  nbins = nblocks * (side/4)^3. */
ZS_ROCM_EXPORT void zs_rocm_mpm_bin_particles(zs_rocm_policy *, const zs_rocm_bht_3 *, zs_rocm_attr pos, size_t n,
                                              float dx, int side, int keyIsOrigin, int *order, int *binStart,
                                              unsigned *cellCount);
/* nbr[b][8]: block numbers of b + {0,1}^3 (x-major), -1 when absent */
ZS_ROCM_EXPORT void zs_rocm_mpm_build_neighbors(zs_rocm_policy *, const zs_rocm_bht_3 *, int *nbr, int keyStride);

/* pol(range(n), P2GTransfer{apic, dt, model, particles, table, grids})
 * (simulation/transfer/P2G.hpp:27-132, cuda/simulation/transfer/P2G.hpp:13-123).
 * binStart/cellCount/nbr == NULL: particle-order path (hash query + global float atomics per node, the
 * reference algorithm); otherwise the binned path: particles must be physically ordered by `order` of
 * zs_rocm_mpm_bin_particles; one wavefront per bin accumulates in registers + LDS and flushes once.  Particles
 * that moved out of their cell since binning are detected and take the particle-order path: results do not
 * depend on the freshness of the bins.  nblocks = number of grid blocks (table size). */
ZS_ROCM_EXPORT void zs_rocm_mpm_p2g(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles,
                                    const zs_rocm_bht_3 *, float *grid, size_t nblocks, const int *binStart,
                                    const unsigned *cellCount, const int *nbr);
/* pol(Collapse{nblocks, side^3}, ComputeGridBlockVelocity{grids, dt, extf, maxVel})
 * (simulation/grid/GridOp.hpp:71-108).  maxVelSqr may be NULL. */
ZS_ROCM_EXPORT void zs_rocm_mpm_grid_update(zs_rocm_policy *, const zs_rocm_mpm_params *, float *grid, size_t nblocks,
                                            const float extf[3], float *maxVelSqr);
/* Collider<AnalyticLevelSet<Plane|Cuboid|Sphere|Cylinder, f32, 3>> (geometry/Collider.h:10-206; the analytic members of
 * GeneralBoundary, :246-252).  param: plane {origin xyz, normal xyz}; cuboid {min xyz, max xyz}; sphere {centre xyz, radius};
 * cylinder {bottom centre xyz, radius, length, axis 0|1|2}.  x = R s X + b maps material to world space (R row-major). */
enum { ZS_ROCM_GEOM_PLANE = 0, ZS_ROCM_GEOM_CUBOID = 1, ZS_ROCM_GEOM_SPHERE = 2, ZS_ROCM_GEOM_CYLINDER = 3 };
enum { ZS_ROCM_COLLIDER_STICKY = 0, ZS_ROCM_COLLIDER_SLIP = 1, ZS_ROCM_COLLIDER_SEPARATE = 2 }; /* collider_e */
typedef struct zs_rocm_collider {
  int geometry, type;
  float param[8];
  float s, dsdt;
  float R[9];
  float omega[3];
  float b[3], dbdt[3];
} zs_rocm_collider;
/* identity transform, sticky */
ZS_ROCM_EXPORT void zs_rocm_collider_init(zs_rocm_collider *c, int geometry, int type, const float *param, int nparam);
/* pol(Collapse{nblocks, side^3}, ApplyBoundaryConditionOnGridBlocks{collider, partition, grids}) (simulation/grid/GridOp.hpp:111-164):
 * every node with mass > 0 at world position (block key * side + cell) * dx gets collider.resolveCollision(pos, vel).
 * Runs after zs_rocm_mpm_grid_update (the grid holds velocities). */
ZS_ROCM_EXPORT void zs_rocm_mpm_apply_boundary(zs_rocm_policy *, const zs_rocm_mpm_params *, const zs_rocm_bht_3 *, float *grid,
                                               size_t nblocks, const zs_rocm_collider *collider);
/* bulk Collider::resolveCollision on n points (x, v: [n][3] device arrays, v updated; inside[n] may be NULL): test entry */
ZS_ROCM_EXPORT void zs_rocm_collider_resolve(zs_rocm_policy *, const zs_rocm_collider *collider, const float *x, float *v, size_t n,
                                             int *inside);
/* Gather-style transfers: linear particle <-> cell-centre weights, 1/8 cell <-> node weights.
 * pol(Collapse{nblocks, side^3}, P2C2GTransfer{scheme, dt, model, buckets, particles, table, grids}): kind 0 = P2C2GTransfer
 * (simulation/transfer/P2C2G.hpp:29-305: mass, momentum with the affine term, and -dt * stress), 1 = P2C2GTransferMomentum (:321-506: mass and
 * momentum only), 2 = P2C2GTransferForce (:522-790: -dt * stress only).  ADDS into grid channels 0..3 (m, mv) like the reference's atomics.
 * `buckets` = zs_rocm_index_buckets_for_particles(pos, n, dx, displacement 0) or zs_rocm_index_buckets_for_partition(...) over this table;
 * particles.C is the reference's `B` (Structurefree.hpp:268-271: one storage).  Built from gathers only (per bucket -> per particle -> per
 * 2x2x2 cells -> per node): no float atomics, reproducible bit for bit; each particle's constitutive update runs once (the reference functor repeats it, and its logJp store, for every cell that sees the particle).
 * Returns 0, -1 on bad arguments. */
ZS_ROCM_EXPORT int zs_rocm_mpm_p2c2g(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_index_buckets *buckets,
                                     const zs_rocm_bht_3 *, float *grid, size_t nblocks, int kind);
/* pol(range(n), PreG2C2PTransfer{particles}) (simulation/transfer/G2C2P.hpp:208-221): v = 0, C = 0 */
ZS_ROCM_EXPORT void zs_rocm_mpm_pre_g2c2p(zs_rocm_policy *, zs_rocm_particles);
/* pol(Collapse{nblocks, side^3}, G2C2PTransfer{scheme, dt, model, buckets, grids, table, particles}) (G2C2P.hpp:38-204): v_p += sum W v_c,
 * B_p += sum W (v_c (x) x_i - v_c (x) x_p); `buckets` may be NULL (the particle side is a gather here). */
ZS_ROCM_EXPORT int zs_rocm_mpm_g2c2p(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_index_buckets *buckets,
                                     const zs_rocm_bht_3 *, const float *grid, size_t nblocks);
/* pol(range(n), PostG2C2PTransfer{scheme, dt, dx, model, particles}) (G2C2P.hpp:224-275): C = B Dinv; F <- (I + dt C) F (J for the fluid);
 * x += v dt */
ZS_ROCM_EXPORT void zs_rocm_mpm_post_g2c2p(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles);
/* The three G2C2P functors above in one pass over the particles (v and B start from 0 instead of being zeroed, re-read and re-written):
 * same bits as zs_rocm_mpm_pre_g2c2p + zs_rocm_mpm_g2c2p + zs_rocm_mpm_post_g2c2p. */
ZS_ROCM_EXPORT int zs_rocm_mpm_g2c2p_step(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                          const float *grid, size_t nblocks);
/* pol(range(n), G2PTransfer{apic, dt, model, grids, table, particles}) (simulation/transfer/G2P.hpp:24-90) */
ZS_ROCM_EXPORT void zs_rocm_mpm_g2p(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles,
                                    const zs_rocm_bht_3 *, const float *grid, size_t nblocks, const int *binStart,
                                    const unsigned *cellCount, const int *nbr);
/* ---- the implicit-MPM system (zpc_amd/csrc/mpm_implicit.hip, mpm_implicit_project.hip).
 * NAMING: the reference's `G2P2GTransfer` functor is the operator below -- internal grid forces at a TRIAL grid velocity, no particle
 * attribute written.  The `zs_rocm_mpm_g2p2g*` entry points further down are something else: the fused EXPLICIT step (G2P of step n +
 * P2G of step n + 1, particles advected and stored).
 * Dof vectors are plain float device arrays [nblocks * side^3][3]: entry 3 * (block * side^3 + cell) + d, the layout of
 * dof_view<space, 3>(Vector<float>) (G2P2G.hpp:71,135-139).  Particles in compact (unslotted) storage.  Every int-returning call
 * validates its arguments first and returns -1 with nothing written, else 0. */
/* pol(range(n), G2P2GTransfer{apic, dt, model, grid, vIn, fOut, table, particles}) (simulation/transfer/G2P2G.hpp:14-150): per particle
 * C from vIn on the stencil of the unchanged position, F_trial = (I + dt C) F (fluid: J_trial = (1 + dt tr C) J), the model on the
 * trial state, W (P F^T vol D_inv) (x_i - x_p) ADDED into fOut.  binStart / cellCount / nbr all NULL: particle order (hash query and
 * global float atomics per node; the gather's sums are formed in the binned kernel's sum-factorised order, not node by node, so that a
 * particle gets the same trial state and stress on either path); all given (zs_rocm_mpm_bin_particles, zs_rocm_mpm_build_neighbors): one workgroup per grid block,
 * results do not depend on how fresh the bins are.  The reference's `grid` argument is not read and is left out.
 * trial: NULL, or float[n][27] = {C_trial:9, F_trial:9 before any plastic projection (fluid: J_trial in slot 0), P F^T vol:9 before
 * D_inv} written per particle (test hook). */
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_force(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                              size_t nblocks, const int *binStart, const unsigned *cellCount, const int *nbr,
                                              const float *vIn, float *fOut, float *trial);
/* ImplicitMPMSystem::multiply (simulation/mpm/ImplicitMPM.hpp:33-59): out := 0, the force operator, then on every entry whose node has
 * grid mass > 0 out[i] = (out[i] dt dt + m) vIn[i] (ForceDtSqrPlusMass :16-31, element-wise as written). */
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_multiply(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                                 const float *grid, size_t nblocks, const int *binStart, const unsigned *cellCount,
                                                 const int *nbr, const float *vIn, float *out);
/* ImplicitMPMSystem::project (Projector, simulation/mpm/ImplicitMPM.hpp:61-124): collider.resolveCollision(pos, vel) on nodes with
 * mass > 0, pos = (key * side + cell) * dx as zs_rocm_mpm_apply_boundary forms it; nodes without mass are zeroed.  collider NULL: only
 * the zeroing. */
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_project(zs_rocm_policy *, const zs_rocm_mpm_params *, const zs_rocm_bht_3 *, const float *grid,
                                                size_t nblocks, const zs_rocm_collider *collider, float *inout);
/* ImplicitMPMSystem::precondition (DivPernodeMass, simulation/mpm/ImplicitMPM.hpp:126-152): out = in / m where m > 0 (IEEE division),
 * other entries untouched */
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_precondition(zs_rocm_policy *, const float *grid, size_t nblocks, int side, const float *in,
                                                     float *out);
/* dof-vector operators on n floats (math/linear/LinearOperators.hpp:14-72): DofAssign{a, b} (b := a), DofFill{a, v},
 * DofCompwiseOp{op}(a, b, c) with op 0 plus, 1 multiplies, 2 minus, 3 divides (-1 for any other op), LinearCombineOp: c = m a + n_ b.
 * A NULL policy or vector: nothing is touched (-1 from zs_rocm_dof_compwise, a plain return from the void calls). */
ZS_ROCM_EXPORT void zs_rocm_dof_assign(zs_rocm_policy *, const float *a, float *b, size_t n);
ZS_ROCM_EXPORT void zs_rocm_dof_fill(zs_rocm_policy *, float *a, float v, size_t n);
ZS_ROCM_EXPORT int zs_rocm_dof_compwise(zs_rocm_policy *, int op, const float *a, const float *b, float *c, size_t n);
ZS_ROCM_EXPORT void zs_rocm_dof_linear_combine(zs_rocm_policy *, float m, const float *a, float n_, const float *b, float *c, size_t n);
/* ConjugateGradient::dotProduct (math/linear/ConjugateGradient.hpp:60-69) without the temporary of products: *out (device) = sum a_i b_i */
ZS_ROCM_EXPORT void zs_rocm_dof_dot(zs_rocm_policy *, const float *a, const float *b, size_t n, float *out);
/* ConjugateGradient::solve (math/linear/ConjugateGradient.hpp:72-161) on the system above: A = multiply, projection with `collider`
 * (may be NULL), preconditioner = division by the node mass.  x: start value in, solution out; *iters (host, may be NULL): iterations
 * run.  maxIters 0 returns with x unchanged.  The reference's debug prints and its getchar() (:158) are left out. */
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_solve(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                              const float *grid, size_t nblocks, const int *binStart, const unsigned *cellCount,
                                              const int *nbr, const zs_rocm_collider *collider, const float *b, float *x, int maxIters,
                                              float tol, float relTol, int *iters);
/* ---- sparse level-set colliders (include/zensim_rocm/levelset_device.hpp, zpc_amd/csrc/levelset.hip): LevelSetBoundary<SparseGrid<3>>, the
 * first member of GeneralBoundary (geometry/Collider.h:246-252), as the boundary of the two grid passes that take one.
 * The level set: a SparseGrid<3, f32, 8> -- `table` a bht<int, 3, int, 16> keyed by block ORIGINS (multiples of 8, index space), `tiles`
 * the data of a TileVector<f32, 512> with numChannels channels and room for numBlocks blocks -- holding "sdf" in channel sdfChannel and,
 * when velChannel >= 0, "v" in channels velChannel .. velChannel + 2.  index = (world - origin) / h.  Cells of absent blocks read as
 * `background` (every channel, as the reference's sampling does).  getSignedDistance / getNormal / getMaterialVelocity:
 * geometry/SparseGrid.hpp:520-545 (linear kernel; normal = central differences at +- h / 4, normalised).
 * stats: NULL, or 4 device words the block kernels ADD to, one count per grid block and launch: [0] blocks culled (no staged sdf value is
 * negative: a trilinear field of non-negative values has no interior point), [1] blocks evaluated from the staged footprint, [2] blocks
 * evaluated by direct hash queries (footprint over the staging budget), [3] unused. */
typedef struct zs_rocm_levelset {
  zs_rocm_bht_view_lite table;
  const float *tiles;
  size_t numBlocks;
  int numChannels, sdfChannel, velChannel;
  float h;
  float origin[3];
  float background;
  unsigned *stats;
} zs_rocm_levelset;
/* The int-returning calls below validate their arguments first and return -1 with nothing written (a level set needs table and tiles,
 * channels inside numChannels, h > 0; a collider used with one needs a type 0..2 and s != 0), else 0. */
/* bulk sampling at n world-space points x[n][3] (test hook): sdf[n], normal[n][3], vel[n][3]; each output may be NULL */
ZS_ROCM_EXPORT int zs_rocm_levelset_sample(zs_rocm_policy *, const zs_rocm_levelset *, const float *x, size_t n, float *sdf, float *normal,
                                           float *vel);
/* bulk Collider<LevelSet>::resolveCollision (geometry/Collider.h:80-110) on n points, like zs_rocm_collider_resolve: `collider` gives type
 * and motion (s, dsdt, R, omega, b, dbdt; geometry and param are not read), the level set the signed distance, the normal and the
 * R s getMaterialVelocity(X) term of v_object.  inside[n] may be NULL. */
ZS_ROCM_EXPORT int zs_rocm_levelset_collider_resolve(zs_rocm_policy *, const zs_rocm_collider *collider, const zs_rocm_levelset *, const float *x,
                                                     float *v, size_t n, int *inside);
/* zs_rocm_mpm_apply_boundary with a level-set collider: one workgroup per grid block stages the block's footprint in the level set into
 * LDS; every node gets the bits zs_rocm_levelset_collider_resolve gives at (key * side + cell) * dx */
ZS_ROCM_EXPORT int zs_rocm_mpm_apply_boundary_levelset(zs_rocm_policy *, const zs_rocm_mpm_params *, const zs_rocm_bht_3 *, float *grid,
                                                       size_t nblocks, const zs_rocm_collider *collider, const zs_rocm_levelset *);
/* zs_rocm_mpm_implicit_project with a level-set collider; collider and level set both NULL: only the zeroing */
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_project_levelset(zs_rocm_policy *, const zs_rocm_mpm_params *, const zs_rocm_bht_3 *, const float *grid,
                                                         size_t nblocks, const zs_rocm_collider *collider, const zs_rocm_levelset *,
                                                         float *inout);
/* zs_rocm_mpm_implicit_solve projecting with a level-set collider (the same driver; collider and level set both NULL: no collider) */
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_solve_levelset(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                                       const float *grid, size_t nblocks, const int *binStart, const unsigned *cellCount,
                                                       const int *nbr, const zs_rocm_collider *collider, const zs_rocm_levelset *,
                                                       const float *b, float *x, int maxIters, float tol, float relTol, int *iters);
/* ---- keyframed level-set colliders (include/zensim_rocm/levelset_device.hpp: TransitionLevelSetView; zpc_amd/csrc/levelset_transition.hip):
 * the blend of two level sets a keyframe spacing stepDt apart at the phase alpha between them, the reference's TransitionLevelSetView
 * over the two front entries of its keyframe queue (geometry/LevelSet.h).  With v = (src.v(x) + dst.v(x)) / 2, x0 = x - alpha stepDt v and
 * x1 = x + (1 - alpha) stepDt v every level-set call is (1 - alpha) src.call(x0) + alpha dst.call(x1); a level set without "v" counts as
 * v = 0.  The float32 operation order is fixed in levelset_device.hpp.  src and dst may be the same level set (a queue of one keyframe).
 * maxSpeed: an upper bound of |v_d| over both level sets' "v" cells and backgrounds (zs_rocm_levelset_max_speed).  It only sizes the
 * block kernels' staged footprints: a cell outside a staged box is read from the grid, so every evaluated node gets the same bits
 * whatever the bound, and a bound that is too large only costs time.  The cull takes the footprint to hold every read: a bound that is
 * too SMALL by more than the footprint's pad (displacements over ~1.75 cells beyond it) may cull a block that holds an inside node.
 * The block kernels add their per-block path counts to src.stats (NULL: not counted), FOUR device words -- all four are written, unlike
 * the single level set's three: [0] culled, [1] evaluated with both sdf boxes staged, [2] evaluated with at least one level set read
 * through direct hash queries, [3] those of [1] where a "v" box did not fit the LDS budget and was read directly.
 * The cull trusts maxSpeed: a block is culled when neither staged sdf box holds a negative value, and the boxes cover the displaced
 * samples only if maxSpeed really bounds |v_d|.  A bound that is too LARGE costs time only.  One that is too SMALL leaves every evaluated
 * node's bits as they are, but once the real displacement exceeds the box's pad (1.75 cells + the widening) a block holding an inside
 * node can be culled: fill maxSpeed from zs_rocm_levelset_max_speed and the backgrounds, never from a guess. */
typedef struct zs_rocm_levelset_transition {
  zs_rocm_levelset src, dst;
  float stepDt, alpha, maxSpeed;
} zs_rocm_levelset_transition;
/* The calls below validate first and return -1 with nothing written: both level sets as above, alpha in [0, 1], stepDt and maxSpeed
 * finite and >= 0. */
/* *out (one device word) = the largest |v_d| over the three "v" channels of all cells of all stored blocks, 0 without "v" (the
 * reference's get_level_set_max_speed samples at the cell centres, which returns the cell values) */
ZS_ROCM_EXPORT int zs_rocm_levelset_max_speed(zs_rocm_policy *, const zs_rocm_levelset *, float *out);
/* zs_rocm_levelset_sample / zs_rocm_levelset_collider_resolve on the transition */
ZS_ROCM_EXPORT int zs_rocm_levelset_transition_sample(zs_rocm_policy *, const zs_rocm_levelset_transition *, const float *x, size_t n, float *sdf,
                                                      float *normal, float *vel);
ZS_ROCM_EXPORT int zs_rocm_levelset_transition_collider_resolve(zs_rocm_policy *, const zs_rocm_collider *collider,
                                                                const zs_rocm_levelset_transition *, const float *x, float *v, size_t n,
                                                                int *inside);
/* the three grid-pass entries above with the transition as the shape: one workgroup per grid block stages both level sets' footprints,
 * widened by the largest displacement of a sample point; every node gets the bits zs_rocm_levelset_transition_collider_resolve gives */
ZS_ROCM_EXPORT int zs_rocm_mpm_apply_boundary_transition(zs_rocm_policy *, const zs_rocm_mpm_params *, const zs_rocm_bht_3 *, float *grid,
                                                         size_t nblocks, const zs_rocm_collider *collider, const zs_rocm_levelset_transition *);
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_project_transition(zs_rocm_policy *, const zs_rocm_mpm_params *, const zs_rocm_bht_3 *, const float *grid,
                                                           size_t nblocks, const zs_rocm_collider *collider,
                                                           const zs_rocm_levelset_transition *, float *inout);
ZS_ROCM_EXPORT int zs_rocm_mpm_implicit_solve_transition(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                                         const float *grid, size_t nblocks, const int *binStart, const unsigned *cellCount,
                                                         const int *nbr, const zs_rocm_collider *collider,
                                                         const zs_rocm_levelset_transition *, const float *b, float *x, int maxIters, float tol,
                                                         float relTol, int *iters);
/* ---- triangle meshes as colliders (include/zensim_rocm/mesh_device.hpp, zpc_amd/csrc/mesh.hip): the bulk form of
 * `pol(range(n), [bvh = proxy<space>(bvh)](i){ bvh.find_nearest(p, f, cap); })` (LBvhView::find_nearest, container/Bvh.hpp:547-590) with the
 * point-triangle distance of geometry/SpatialQuery.hpp:19-315 (dist_pt_sqr / pt_category_and_dist2) as the functor f, and the conversion
 * of a mesh into the SparseGrid<3, f32, 8> level set of zs_rocm_levelset (the reference does this through OpenVDB,
 * geometry/VdbLevelSet_*.cpp).  The object copies verts [nv][3] f32, tris [nt][3] i32 and the optional per-vertex velocities [nv][3] f32
 * (NULL: none) from device memory and owns: an LBvh over the triangle boxes (zs_rocm_lbvh_build), unit face normals, angle-weighted vertex
 * pseudonormals and edge pseudonormals (sum of the adjacent face normals; an edge with one face: that face's normal).  Edge adjacency:
 * 3 nt half-edge keys (min vertex, max vertex) sorted as u64; vertex sums: corners sorted by vertex, each vertex folds its run in that
 * order -- the same mesh gives the same bits on every run.  Vertex indices outside [0, nv) are clamped and counted.
 * Sign of the distance: (p - closest) . pseudonormal(feature) (Baerentzen & Aanaes 2005); features: 0..2 vertex a/b/c, 3..5 edge ab/bc/ca,
 * 6 face.  Int-returning calls validate their arguments and return -1 with nothing written, else 0. */
typedef struct zs_rocm_mesh zs_rocm_mesh;
typedef struct {
  const float *verts;
  const int *tris;
  const float *vel; /* NULL without velocities */
  const float *faceNormals, *vertNormals, *edgeNormals; /* [nt][3], [nv][3], [nt][3 edges][3] */
  zs_rocm_lbvh_view bvh;
  int numVerts, numTris;
} zs_rocm_mesh_view;
#define ZS_ROCM_MESH_STAT_WORDS 8
ZS_ROCM_EXPORT zs_rocm_mesh *zs_rocm_mesh_create(zs_rocm_policy *, const float *verts, size_t nv, const int *tris, size_t nt, const float *vel);
ZS_ROCM_EXPORT void zs_rocm_mesh_destroy(zs_rocm_mesh *);
/* new vertex positions (and velocities: NULL keeps the old ones) on the same topology: LBvh::refit (Bvh.hpp:1219-1248) + the normals */
ZS_ROCM_EXPORT int zs_rocm_mesh_refit(zs_rocm_policy *, zs_rocm_mesh *, const float *verts, const float *vel);
/* out (host, ZS_ROCM_MESH_STAT_WORDS ints): [0] boundary edges (one face), [1] non-manifold edges (more than two faces), [2] edge pairs
 * whose two faces run along the edge in the same direction, [3] zero-area triangles, [4] vertex indices out of range; synchronises */
ZS_ROCM_EXPORT void zs_rocm_mesh_stats(zs_rocm_policy *, const zs_rocm_mesh *, int *out);
/* box6 (host): LBvh::getTotalBox of the triangle boxes (Bvh.hpp:152-171); synchronises; -1 for a mesh without triangles */
ZS_ROCM_EXPORT int zs_rocm_mesh_total_box(zs_rocm_policy *, const zs_rocm_mesh *, float *box6);
/* all zero for a NULL mesh */
ZS_ROCM_EXPORT void zs_rocm_mesh_get_view(const zs_rocm_mesh *, zs_rocm_mesh_view *out);
/* bulk find_nearest at points [nq][3]: dist[nq], tri[nq], feature[nq], bary[nq][3]; each output may be NULL.  No triangle nearer than
 * cap: dist = cap, tri = feature = -1.  16384 or more points are walked in Morton order of the points, like zs_rocm_lbvh_query_*. */
ZS_ROCM_EXPORT int zs_rocm_mesh_closest_point(zs_rocm_policy *, const zs_rocm_mesh *, const float *points, size_t nq, float cap, float *dist,
                                              int *tri, int *feature, float *bary);
/* sdf[nq] = signed distance (+cap when none is nearer), vel[nq][3] = the vertex velocities interpolated at the closest point; either may
 * be NULL */
ZS_ROCM_EXPORT int zs_rocm_mesh_signed_distance(zs_rocm_policy *, const zs_rocm_mesh *, const float *points, size_t nq, float cap, float *sdf,
                                                float *vel);
/* mesh -> level set.  Cell (i, j, k) sits at origin + voxel (i, j, k) (origin: 3 host floats); the result is what a dense sampling keeps:
 * every 8^3 block with a cell |sdf| < band, all 512 cells of it the signed distance.  The caller owns every container and sizes it from
 * the two counts the calls return:
 *   count       sum over the triangles of the blocks their boxes, dilated by band, touch (synchronises): with the number of blocks in
 *               the mesh's dilated total box, an upper bound for the candidates
 *   candidates  inserts those blocks (keys = block origins, multiples of 8) into `cand`, a bht<int, 3, int, 16>
 *   blocks      one workgroup per candidate, lane = cell: tiles [ncand] x numChannels x 512 (numChannels 1: sdf; 4: sdf, v) and
 *               keep[ncand] = 1 where a cell has |sdf| < band.  The tree is culled once per block against the block's box and the
 *               surviving triangles are staged in LDS; a block with more survivors than the stage holds walks the tree per lane.
 *               stats: NULL or 4 device words ADDED to: [0] blocks rejected by their centre's distance, [1] staged, [2] per-lane, [3] kept
 *   select      keptKeys [<= ncand][3] = keys of the kept blocks; returns their number (synchronises)
 *   gather      the kept blocks' tiles to the place `table` (the final bht, holding exactly the kept keys) gives them */
ZS_ROCM_EXPORT size_t zs_rocm_mesh_levelset_count(zs_rocm_policy *, const zs_rocm_mesh *, const float *origin, float voxel, float band);
ZS_ROCM_EXPORT int zs_rocm_mesh_levelset_candidates(zs_rocm_policy *, const zs_rocm_mesh *, const float *origin, float voxel, float band,
                                                    zs_rocm_bht_3 *cand);
ZS_ROCM_EXPORT int zs_rocm_mesh_levelset_blocks(zs_rocm_policy *, const zs_rocm_mesh *, const float *origin, float voxel, float band,
                                                const zs_rocm_bht_3 *cand, size_t ncand, float *tiles, int numChannels, int *keep,
                                                unsigned *stats);
ZS_ROCM_EXPORT size_t zs_rocm_mesh_levelset_select(zs_rocm_policy *, const zs_rocm_bht_3 *cand, size_t ncand, const int *keep, int *keptKeys);
ZS_ROCM_EXPORT int zs_rocm_mesh_levelset_gather(zs_rocm_policy *, const zs_rocm_bht_3 *cand, size_t ncand, const int *keep, const float *tiles,
                                                const zs_rocm_bht_3 *table, float *dstTiles, int numChannels);
/* ---- mesh proximity pairs (zpc_amd/csrc/mesh_proximity.hip): the vertex-triangle (PT) and edge-edge (EE) pairs of a mesh with itself
 * that are closer than a contact distance dHat, topological neighbours removed (a triangle that contains the vertex, two edges that share
 * a vertex), each with its squared distance and the feature pair it is realised on -- dist_pt_sqr / pt_category_and_dist2 / dist_ee_sqr /
 * ee_category_and_dist2 (geometry/SpatialQuery.hpp:19-500) behind iter_neighbors / self_iter_neighbors, walk and exact test in one kernel.
 *   edges     the unique edges [ne][2] of the mesh, e[0] < e[1], in lexicographic order (from the sorted half-edge keys; an index pair
 *             (i, i) of a degenerate triangle is no edge); zs_rocm_mesh_edges copies them to device memory
 *   count     PT: counts[nv] by vertex; EE: counts[ne] by leaf of the edge tree (built by the first EE call, refitted by
 *             zs_rocm_mesh_refit from then on)
 *   fill      offsets = exclusive scan of the counts.  PT: pairs (vertex, triangle), dist2, feature (0..6 as above), bary [n][3];
 *             EE: pairs (i, j) with i < j, dist2, category = uCate * 3 + vCate (0 first endpoint, 1 second endpoint, 2 interior; u on
 *             edge i), st [n][2] = the parameters of the closest points on edge i and edge j.  Every output may be NULL.
 * The order of the lists is a function of the input alone: two calls give the same bytes.  -1 and nothing written for a NULL mesh or a
 * dHat that is not finite and positive; a mesh without triangles has zero counts. */
ZS_ROCM_EXPORT size_t zs_rocm_mesh_num_edges(const zs_rocm_mesh *);
ZS_ROCM_EXPORT int zs_rocm_mesh_edges(zs_rocm_policy *, const zs_rocm_mesh *, int *edges);
ZS_ROCM_EXPORT int zs_rocm_mesh_proximity_pt_count(zs_rocm_policy *, const zs_rocm_mesh *, float dHat, int *counts);
ZS_ROCM_EXPORT int zs_rocm_mesh_proximity_pt_fill(zs_rocm_policy *, const zs_rocm_mesh *, float dHat, const int *offsets, int *pairs, float *dist2,
                                                  int *feature, float *bary);
ZS_ROCM_EXPORT int zs_rocm_mesh_proximity_ee_count(zs_rocm_policy *, zs_rocm_mesh *, float dHat, int *counts);
ZS_ROCM_EXPORT int zs_rocm_mesh_proximity_ee_fill(zs_rocm_policy *, zs_rocm_mesh *, float dHat, const int *offsets, int *pairs, float *dist2,
                                                  int *category, float *st);
/* ---- mesh barrier potential (zpc_amd/csrc/mesh_barrier.hip, include/zensim_rocm/barrier_device.hpp): the IPC log-barrier contact energy
 * and its gradient (the contact force) over the PT and EE pair lists of the proximity passes -- barrier / barrier_gradient
 * (geometry/SpatialQuery.hpp:502-531) with dist_grad_* and mollifier_ee (geometry/Distance.hpp) -- at the mesh's own positions or at trial
 * positions verts [nv][3] on the same topology (NULL: the mesh's own).  Distance, parameters and feature are recomputed at those positions;
 * a pair at dHat or beyond contributes exactly zero.  b(d2) = -kappa (d2 - dHat^2)^2 log(d2 / dHat^2); an EE pair is multiplied by the
 * mollifier of its edges' cross product against 1e-2 restLen2_i restLen2_j when mollify != 0.
 *   set_rest    stores the squared rest length of every unique edge [ne] in the mesh object, from verts [nv][3] or (NULL) the mesh's current
 *               vertices; zs_rocm_mesh_rest copies them out ([ne], -1 before set_rest)
 *   sizes       sizes[0] = ints of starts (nv + 1), sizes[1] = ints of entries (4 (npt + nee)), sizes[2] = floats of scratch (12 (npt + nee))
 *   incidence   starts / entries of a pair of lists: entries = the (pair, corner) numbers 4 pair + corner (EE pairs numbered behind the PT
 *               pairs) sorted by vertex, list order inside a vertex; starts[v] .. starts[v + 1] is the run of vertex v.  Depends on the
 *               lists alone, not on positions: build once, reuse for every call on the same lists.
 *   energy      ptEnergy [npt], eeEnergy [nee] (float), total (one double, PT then EE, summed in a fixed order), status int[2] = the PT and EE
 *               pairs at zero distance (their energy is +inf, they add nothing to the gradient).  Every output may be NULL.
 *   gradient    the same and grad [nv][3], fully overwritten, zero for a vertex in no pair; scratch holds the per-pair contributions.
 * Two calls on the same input give the same bytes (no float atomics).  -1 and nothing written for a NULL mesh, a dHat or kappa that is not
 * finite and positive, mollify != 0 before set_rest, or 2^28 pairs and more; empty lists give zero energy and a zero gradient. */
ZS_ROCM_EXPORT int zs_rocm_mesh_set_rest(zs_rocm_policy *, zs_rocm_mesh *, const float *verts);
ZS_ROCM_EXPORT int zs_rocm_mesh_rest(zs_rocm_policy *, const zs_rocm_mesh *, float *restLen2);
ZS_ROCM_EXPORT int zs_rocm_mesh_barrier_sizes(const zs_rocm_mesh *, size_t npt, size_t nee, size_t *sizes);
ZS_ROCM_EXPORT int zs_rocm_mesh_barrier_incidence(zs_rocm_policy *, const zs_rocm_mesh *, const int *ptPairs, size_t npt, const int *eePairs,
                                                  size_t nee, int *starts, int *entries);
ZS_ROCM_EXPORT int zs_rocm_mesh_barrier_energy(zs_rocm_policy *, const zs_rocm_mesh *, const float *verts, const int *ptPairs, size_t npt,
                                               const int *eePairs, size_t nee, float dHat, float kappa, int mollify, float *ptEnergy,
                                               float *eeEnergy, double *total, int *status);
ZS_ROCM_EXPORT int zs_rocm_mesh_barrier_gradient(zs_rocm_policy *, const zs_rocm_mesh *, const float *verts, const int *ptPairs, size_t npt,
                                                 const int *eePairs, size_t nee, float dHat, float kappa, int mollify, const int *starts,
                                                 const int *entries, float *scratch, float *ptEnergy, float *eeEnergy, double *total,
                                                 float *grad, int *status);
/* The Hessian-vector product of the same potential over the same lists, matrix-free (the job of barrier_hessian with dist_hess_pp / _pe /
 * _pt / _ee, geometry/Distance.hpp, as an operator): hx [nv][3] = H x for a direction x [nv][3], H the second derivative of the total
 * energy at verts (NULL: the mesh's own).  Per pair (H_pair x) on its four corners goes to scratch (sizes[2] floats, PT pairs first, [4][3]
 * each; the caller may read them), then the gather of mesh_terms.hip sums them per vertex in list order on starts / entries of
 * _barrier_incidence: no float atomics, two calls give the same bytes.  psd != 0: the positive semi-definite H+ of barrier_device.hpp (b'' g g^T + |b'| F^T A^-1 F,
 * mollified: m H+_b + b m' 2 J^T J), a majorant of H without the mollifier; it is not the eigenvalue projection of the 12 x 12 blocks.
 * status as above; a pair at zero distance (or whose b'' or product leaves the float range) contributes zero and is counted.  -1 for the
 * argument errors of _barrier_gradient, or x or hx NULL with nv > 0. */
ZS_ROCM_EXPORT int zs_rocm_mesh_barrier_hessian_product(zs_rocm_policy *, const zs_rocm_mesh *, const float *verts, const int *ptPairs, size_t npt,
                                                        const int *eePairs, size_t nee, float dHat, float kappa, int mollify, int psd,
                                                        const float *x, const int *starts, const int *entries, float *scratch, float *hx,
                                                        int *status);
/* ---- mesh friction (zpc_amd/csrc/mesh_barrier.hip, include/zensim_rocm/friction_device.hpp): lagged IPC friction over the same PT and EE
 * lists -- the smoothed static-friction functions f0_SF / f1_SF_div_rel_dx_norm / f2_SF_term and the tangent bases and relative
 * displacements of geometry/Friction.hpp, with the projector I - n n^T in place of the per-feature bases.
 *   lag       at verts [nv][3] (NULL: the mesh's own positions), the positions the normal forces are frozen at: record [npt + nee][8]
 *             floats, PT pairs first, each n[3] (the unit vector P - Q), lambda = m (-b'(d2)) 2 d (the size of the contact force; dHat,
 *             kappa, mollify as for the barrier) and w[4] (the weights of the relative displacement).  A pair at dHat or beyond, or with
 *             an index outside the mesh, gets an all-zero record; so does a pair at zero distance or with a lambda beyond the float
 *             range, which is counted in status int[2] (PT, EE).
 *   energy    at a displacement u [nv][3] (x - x at the start of the step), with mu >= 0 and the static-friction threshold epsv > 0 in
 *             displacement units, from the record alone:  mu lambda f0(|ut|), ut the tangential part of sum_k w_k u_k.  ptEnergy [npt],
 *             eeEnergy [nee], total (one double, PT then EE, the barrier's fixed order); each may be NULL.  status int[2] = the PT and EE
 *             pairs whose |ut|^2 or result leaves the float range: they contribute exactly zero.
 *   gradient  the same and grad [nv][3], fully overwritten; starts / entries / scratch as for _barrier_gradient (the same incidence).
 *   product   hx [nv][3] = H x for a direction x [nv][3], H the second derivative of the energy at u: positive semi-definite by
 *             construction.  scratch receives the per-pair terms [4][3], PT pairs first.
 * Two calls give the same bytes (no float atomics).  -1 and nothing written for a NULL policy, mesh, record (with pairs) or u, x, hx, grad
 * (with vertices), a list with a count and no pointer, 2^28 pairs and more, a mu that is negative or not finite, an epsv that is not finite
 * and positive, and for the lag step the argument errors of _barrier_energy. */
ZS_ROCM_EXPORT int zs_rocm_mesh_friction_lag(zs_rocm_policy *, const zs_rocm_mesh *, const float *verts, const int *ptPairs, size_t npt,
                                             const int *eePairs, size_t nee, float dHat, float kappa, int mollify, float *record, int *status);
ZS_ROCM_EXPORT int zs_rocm_mesh_friction_energy(zs_rocm_policy *, const zs_rocm_mesh *, const float *u, const int *ptPairs, size_t npt,
                                                const int *eePairs, size_t nee, const float *record, float mu, float epsv, float *ptEnergy,
                                                float *eeEnergy, double *total, int *status);
ZS_ROCM_EXPORT int zs_rocm_mesh_friction_gradient(zs_rocm_policy *, const zs_rocm_mesh *, const float *u, const int *ptPairs, size_t npt,
                                                  const int *eePairs, size_t nee, const float *record, float mu, float epsv, const int *starts,
                                                  const int *entries, float *scratch, float *ptEnergy, float *eeEnergy, double *total,
                                                  float *grad, int *status);
ZS_ROCM_EXPORT int zs_rocm_mesh_friction_hessian_product(zs_rocm_policy *, const zs_rocm_mesh *, const float *u, const float *x,
                                                         const int *ptPairs, size_t npt, const int *eePairs, size_t nee, const float *record,
                                                         float mu, float epsv, const int *starts, const int *entries, float *scratch,
                                                         float *hx, int *status);
/* ---- mesh elasticity (zpc_amd/csrc/mesh_elastic.hip, include/zensim_rocm/elastic_device.hpp): the internal energy of the mesh itself, StVK
 * membrane energy over the triangles (mu, lam: per-area Lame stiffnesses, the thickness multiplied in) plus quadratic bending energy over
 * the hinges (kb), against a rest shape kept in the mesh object; energy, gradient and matrix-free Hessian-vector product in the shape of
 * the contact terms.  The bending energy is zero at rest only where the rest shape is flat across the hinge (cloth); on a curved rest
 * shape it penalises the rest curvature too.
 *   set_rest_shape  from verts [nv][3] or (NULL) the mesh's current vertices: the triangle records [nt][4] (B00, B01, B11, A), the hinges
 *                   [nh][4] (every unique edge with exactly two triangles, in edge order: the edge's vertices v0 < v1, the opposite vertex of
 *                   the incident triangle with the smaller index, that of the other), their records [nh][4] and the vertex areas [nv] (a
 *                   third of the incident rest areas).  Degenerate rest triangles and hinges get all-zero records and contribute nothing.
 *                   A second call recomputes the records and keeps the hinges.
 *   sizes           sizes[0..3] = nt, nh, nv, floats of scratch (9 nt + 12 nh); sizes[4..6] = degenerate triangles, degenerate hinges,
 *                   non-manifold edges (more than two triangles: no hinge) of the last set_rest_shape.  size_t sizes[7].
 *   rest_shape      copies out triRecord [nt][4], hinges [nh][4], hingeRecord [nh][4], vertexArea [nv]; each may be NULL.
 *   energy          triEnergy [nt], hingeEnergy [nh] (float), total (one double, triangles then hinges, summed in a fixed order), status
 *                   int[2] = the triangles and hinges whose result leaves the float range (they contribute exactly zero).  Every output
 *                   may be NULL.  verts NULL: the mesh's own positions.
 *   gradient        the same and grad [nv][3], fully overwritten; scratch holds the per-element terms, [nt][3][3] then [nh][4][3].
 *   product         hx [nv][3] = H x for the direction x [nv][3]; psd != 0: the positive semi-definite H+ (the membrane stress projected
 *                   onto the positive semi-definite matrices in closed form), a majorant of H that equals it where no triangle is compressed.
 * mu = lam = 0 skips the membrane, kb = 0 the bending; both then contribute exactly zero.  Two calls give the same bytes (no float
 * atomics).  -1 and nothing written for a NULL policy, mesh, x, hx, grad (with vertices) or scratch (with elements), a stiffness that is
 * negative or not finite, or before set_rest_shape. */
ZS_ROCM_EXPORT int zs_rocm_mesh_set_rest_shape(zs_rocm_policy *, zs_rocm_mesh *, const float *verts);
ZS_ROCM_EXPORT int zs_rocm_mesh_rest_shape_sizes(const zs_rocm_mesh *, size_t *sizes);
ZS_ROCM_EXPORT int zs_rocm_mesh_rest_shape(zs_rocm_policy *, const zs_rocm_mesh *, float *triRecord, int *hinges, float *hingeRecord,
                                           float *vertexArea);
ZS_ROCM_EXPORT int zs_rocm_mesh_elastic_energy(zs_rocm_policy *, const zs_rocm_mesh *, const float *verts, float mu, float lam, float kb,
                                               float *triEnergy, float *hingeEnergy, double *total, int *status);
ZS_ROCM_EXPORT int zs_rocm_mesh_elastic_gradient(zs_rocm_policy *, const zs_rocm_mesh *, const float *verts, float mu, float lam, float kb,
                                                 float *scratch, float *triEnergy, float *hingeEnergy, double *total, float *grad, int *status);
ZS_ROCM_EXPORT int zs_rocm_mesh_elastic_hessian_product(zs_rocm_policy *, const zs_rocm_mesh *, const float *verts, float mu, float lam,
                                                        float kb, int psd, const float *x, float *scratch, float *hx, int *status);
/* ---- mesh Newton system (zpc_amd/csrc/mesh_solve.hip, include/zensim_rocm/solve_device.hpp): the linear system of one Newton iteration of
 * the incremental potential, A = diag(mass) + scale (H+_elastic + H+_barrier + H_friction) on [nv][3] float32 vectors (scale = h^2 for
 * backward Euler), its per-vertex 3 x 3 diagonal blocks, the operator and a block-Jacobi preconditioned conjugate-gradient solve whose
 * scalars stay on the device.  The terms are the products above with psd != 0 (friction as it stands); each is optional.
 *   descriptor  mass [nv]; fixed [nv] bytes or NULL (non-zero: a Dirichlet vertex; a vertex whose mass is not finite and positive is
 *               treated as fixed too); scale (finite; a negative one is accepted and makes the solve break down); elastic != 0: mu, lam,
 *               kb as for the elastic product; barrier != 0: the two lists, their incidence (zs_rocm_mesh_barrier_incidence), dHat, kappa,
 *               mollify; friction != 0: the displacement u [nv][3], the lag step's lists (they may differ from the barrier's), their
 *               incidence, the records, fmu, epsv.  verts: the trial positions of the elastic and the barrier term, NULL: the mesh's own.
 *   sizes       sizes[0] = floats of scratch for multiply and solve (the per-element terms: elastic, barrier, friction, one behind the
 *               other), sizes[1] = floats of scratch for blocks (twice that: six floats per corner), sizes[2] = nv.  size_t sizes[3].
 *   blocks      a block is 6 floats (xx, xy, xz, yy, yz, zz); entry (i, j), i <= j, of a term's block at v is component i at v of that
 *               term's product with the unit direction e_{v,j}, value for value: element kernels write every element's own corner blocks
 *               with the product's own device function, a gather sums them per vertex in the product's run order.  elastic, barrier,
 *               friction [nv][6]: the per-term blocks (zeros for a term that is absent); combined [nv][6] = scale ((elastic + barrier) +
 *               friction) plus the mass on the diagonal; inverse [nv][6]: its inverse in closed form, the scalar Jacobi where that fails
 *               (solve_device.hpp), zero at a fixed vertex.  status int[8] = elastic overflows (triangles, hinges), barrier zero-distance
 *               pairs (PT, EE), friction overflows (PT, EE), inverse fallbacks, masses treated as fixed.  All five arrays are required.
 *   multiply    q = A x: the element kernels of the three products write their per-element terms to scratch as they do in the product
 *               calls, then one gather per vertex sums the elastic triangle run, the elastic hinge run, the barrier run and the friction
 *               run into one float32 accumulator, each run front to back; q_v = mass_v x_v + scale acc_v, zero at a fixed vertex.
 *   solve       preconditioned CG from x (in: the start, out: the solution) for the right-hand side b, z = inverse r, res = sqrt(r . z),
 *               stopping at res <= min(relTol res0, tol) or after maxIters iterations.  Dot products: every product of two floats exact in
 *               float64, summed in float64 in a fixed order; alpha and beta are float64 quotients rounded to float32 once on the device.
 *               record: 2 + maxIters + 1 words on the device = iters (int), flag (int), the residual history (float, entry k after k
 *               iterations).  flag: 1 converged, 2 maxIters reached, 3 breakdown (p . A p not positive), 4 a scalar that is not finite.
 *               Once the flag is set x, iters and the history no longer change.  The host enqueues checkEvery >= 1 iterations at a time
 *               and reads the flag once per batch; the result does not depend on checkEvery.
 * Two calls give the same bytes (no float atomics).  -1 and nothing written for a NULL policy, mesh, descriptor, mass (with vertices) or
 * output, whatever the sibling product call of a term that is present rejects, a scale that is not finite, maxIters < 0, checkEvery < 1. */
typedef struct zs_rocm_mesh_system {
  const float *mass;
  const unsigned char *fixed;
  float scale;
  const float *verts;
  int elastic;
  float mu, lam, kb;
  int barrier;
  const int *ptPairs;
  size_t npt;
  const int *eePairs;
  size_t nee;
  const int *starts, *entries;
  float dHat, kappa;
  int mollify;
  int friction;
  const float *u;
  const int *fPtPairs;
  size_t fNpt;
  const int *fEePairs;
  size_t fNee;
  const int *fStarts, *fEntries;
  const float *record;
  float fmu, epsv;
} zs_rocm_mesh_system;
ZS_ROCM_EXPORT int zs_rocm_mesh_system_sizes(const zs_rocm_mesh *, const zs_rocm_mesh_system *, size_t *sizes);
ZS_ROCM_EXPORT int zs_rocm_mesh_system_blocks(zs_rocm_policy *, const zs_rocm_mesh *, const zs_rocm_mesh_system *, float *scratch, float *elastic,
                                              float *barrier, float *friction, float *combined, float *inverse, int *status);
ZS_ROCM_EXPORT int zs_rocm_mesh_system_multiply(zs_rocm_policy *, const zs_rocm_mesh *, const zs_rocm_mesh_system *, float *scratch,
                                                const float *x, float *q);
ZS_ROCM_EXPORT int zs_rocm_mesh_system_solve(zs_rocm_policy *, const zs_rocm_mesh *, const zs_rocm_mesh_system *, float *scratch,
                                             const float *inverse, const float *b, float *x, int maxIters, float tol, float relTol,
                                             int checkEvery, void *record);
/* ---- mesh incremental potential (zpc_amd/csrc/mesh_potential.hip, include/zensim_rocm/potential_device.hpp): the objective the Newton system
 * above linearises, E(x) = 1/2 (x - target)^T M (x - target) + scale (Psi_elastic(x) + B(x) + D(x - start)), as one fused evaluation of energy
 * and gradient and as a backtracking line search whose decisions stay on the device.  The terms come in a zs_rocm_mesh_system descriptor
 * (mass, fixed, scale and the three optional terms as above; its verts and u are not read: the entries take the positions verts [nv][3],
 * the inertia target [nv][3] and, required with friction, the positions start [nv][3] at the start of the step, u = verts - start).  The
 * barrier's lists may be any proximity lists of the mesh with a radius of at least dHat: a pair at dHat or beyond adds exactly nothing.
 *   sizes        sizes[0] = floats of scratch (the per-element gradient terms, laid out as for the system's multiply), sizes[1] = floats of
 *                energies (one per vertex, then one per triangle, hinge, barrier pair, friction pair of the terms present), sizes[2] = nv.
 *   evaluate     parts double[5] on the device = the inertia, elastic, barrier and friction energies, each the float64 fixed-order total of
 *                its float32 per-element energies in the order of the public energy calls (whose totals they equal bit for bit), then
 *                E = parts[0] + (double) scale ((parts[1] + parts[2]) + parts[3]).  grad [nv][3] or NULL (energy only: no scratch needed):
 *                g = mass (x - target) + scale acc, acc one float32 accumulator over the elastic triangle run, the elastic hinge run, the
 *                barrier run and the friction run of the vertex, each front to back; a fixed vertex has no inertia energy and a zero row.
 *                status int[6] or NULL = elastic overflows (triangles, hinges), barrier zero-distance pairs (PT, EE), friction overflows.
 *   line_search  backtracking from verts along dir [nv][3]: t_0 = tMax (tMaxDev != NULL: one device float, read in its place), t_{k+1} =
 *                shrink t_k, x_k = verts + t_k dir (verts at a fixed vertex); trial k is accepted iff E_k is finite and
 *                E_k <= E_0 + ((double) c1 (double) t_k) slope, slope = grad . dir in float64.  record on the device: int trials, int flag,
 *                float t (the accepted step, else 0), float (the next trial's step), double energy (of the accepted trial, else E_0),
 *                double slope, double history[maxTrials + 1] (E_0, then one entry per trial): 32 + 8 (maxTrials + 1) bytes.  flag: 1
 *                accepted, 2 maxTrials reached, 3 slope not negative, 4 E_0, slope or tMax not finite or tMax <= 0.  x [nv][3]: the accepted
 *                trial, else a copy of verts; it must not alias verts or dir.  Once the flag is set nothing of the record changes.  The host
 *                enqueues checkEvery >= 1 trials at a time and reads the flag once per batch; the result does not depend on checkEvery.
 *                No collision check is made: a trial across a pair has a finite barrier energy again, so tMax has to come from
 *                zs_rocm_mesh_ccd.
 * Two calls give the same bytes (no float atomics).  -1 and nothing written for a NULL policy, mesh, descriptor, mass, target, verts (with
 * vertices) or output, friction without start, whatever the system entries reject, c1 negative or not finite, shrink outside (0, 1),
 * maxTrials < 1, checkEvery < 1. */
ZS_ROCM_EXPORT int zs_rocm_mesh_potential_sizes(const zs_rocm_mesh *, const zs_rocm_mesh_system *, size_t *sizes);
ZS_ROCM_EXPORT int zs_rocm_mesh_potential_evaluate(zs_rocm_policy *, const zs_rocm_mesh *, const zs_rocm_mesh_system *, const float *target,
                                                   const float *start, const float *verts, float *scratch, float *energies, double *parts,
                                                   float *grad, int *status);
ZS_ROCM_EXPORT int zs_rocm_mesh_potential_line_search(zs_rocm_policy *, const zs_rocm_mesh *, const zs_rocm_mesh_system *, const float *target,
                                                      const float *start, const float *verts, const float *dir, float tMax,
                                                      const float *tMaxDev, float c1, float shrink, int maxTrials, int checkEvery,
                                                      float *scratch, float *energies, float *x, void *record);
/* ---- mesh CCD (zpc_amd/csrc/mesh_ccd.hip, include/zensim_rocm/ccd_device.hpp): a conservative bound on the step t in [0, tMax] for which
 * verts + t dir (verts NULL: the mesh's own positions; dir [nv][3]) keeps every pair of the two lists free of contact, by additive CCD on
 * the unsigned distance -- what a line search needs before it may evaluate the barrier.  The reference has yes / no tests only
 * (vertexFaceCCD / edgeEdgeCCD, geometry/Geometry.hpp; pt_ccd_broadphase / ee_ccd_broadphase, geometry/AnalyticLevelSet.h).  Per pair the
 * step keeps the distance above slack x its value at t = 0; ptToi [npt] / eeToi [nee] receive the per-pair bounds (NULL: not wanted), tMin
 * (one device float) their minimum and tMax, status int[4] = the pairs at zero distance PT, EE (their bound is 0), then the pairs stopped
 * by maxIter distance evaluations PT, EE (their bound is valid, not tight).  A pair with an index outside the mesh gets tMax, a pair with a
 * NaN or Inf in its rows 0.  Two calls give the same bytes; the outputs do not depend on the order of the lists.  -1 and nothing written
 * for a NULL policy, mesh, dir or tMin, slack outside (0, 1), a tMax that is not finite and positive, maxIter < 1, a list with a count
 * and no pointer, or 2^28 pairs and more; with both lists empty tMin = tMax. */
ZS_ROCM_EXPORT int zs_rocm_mesh_ccd(zs_rocm_policy *, const zs_rocm_mesh *, const float *verts, const float *dir, const int *ptPairs, size_t npt,
                                    const int *eePairs, size_t nee, float slack, float tMax, int maxIter, float *ptToi, float *eeToi,
                                    float *tMin, int *status);
/* ---- slotted particle storage: the motion-robust form of the fused step (zpc_amd/csrc/mpm_slotted.hip).  Storage = bins x K rounds x
 * 64 lanes in ONE TileVector<f32, 64> (slot (bin, r, lane) = element (bin K + r) 64 + lane), cellMask[bin][lane] = occupied rounds of the
 * cell; a particle is always stored under the cell of its base node, and the step keeps it so.  A particle that changes cell is finished
 * by the workgroup that moves it: inside the bin it draws a ticket for the lowest free round of its new cell and is scattered by that
 * cell's lane; across bins its grid terms are added by global float atomics and a record goes to the bin's outbox (outboxCap records
 * per bin), from where a second, small kernel copies it into a free round of the destination cell (one ticket per record on claim[]),
 * and a third folds tickets and departures into cellMask.  No re-bin, no exact-path queues in the time loop.  Buffers: moverCount (int),
 * claim (unsigned; zeroed by the caller ONCE, every step leaves it zero), moverRec (float) -- their sizes in bytes come from
 * zs_rocm_mpm_slot_outbox_bytes(nbins, outboxCap, which = 0 / 1 / 2).  status: int[ZS_ROCM_SLOT_STATUS_WORDS], zeroed by the caller,
 * latched: [0] an outbox was full, [1] a
 * cell ran out of rounds, [2] mass or a mover for a block outside the partition, [3] early warning: a particle lives in a block flagged by
 * blockEdge (re-partition within `side` steps), [4] a particle was not stored under its cell, or moved more than one cell in a step;
 * [8, 264) and [264, 520): movers sent / re-homed (running sums spread over 256 words each: a single device-wide word would serialise one
 * atomic per bin); the totals are equal after every step.  NO PARTICLE IS EVER DROPPED (the reference writes every particle back,
 * G2P.hpp:67-82): a mover that finds its outbox full, its new cell full (inside the bin or, r04, in another bin: slot_rehome_kernel puts
 * it back), its destination block missing from the partition (r04), or that has moved more than a cell KEEPS its old slot with its new
 * state; it is then stored under the wrong cell and skipped ([4]) until the caller re-slots the storage (unslot / re-partition / slot),
 * which the flags [0], [1], [2] ask for.  Only GRID contributions can be dropped ([2]: a stencil node whose block is missing; the
 * reference does not check that either, P2G.hpp:109-110).
 * The per-particle arithmetic is that of zs_rocm_mpm_g2p2g (G2P.hpp:44-83 + P2G.hpp:51-125). */
#define ZS_ROCM_SLOT_STATUS_WORDS (8 + 2 * 256)
ZS_ROCM_EXPORT size_t zs_rocm_mpm_slot_outbox_bytes(size_t nbins, int outboxCap, int which); /* 0 moverCount, 1 claim words, 2 moverRec */
ZS_ROCM_EXPORT void zs_rocm_mpm_build_neighbors27(zs_rocm_policy *, const zs_rocm_bht_3 *, int *nbr27 /* [nblocks][27] */, int keyStride);
/* src: TileVector<f32,64> with C channels and n particles in any order -> dst: nbins*K tiles; status: int[ZS_ROCM_SLOT_STATUS_WORDS] ([1], [2] are used here) */
ZS_ROCM_EXPORT int zs_rocm_mpm_slot_particles(zs_rocm_policy *, const zs_rocm_bht_3 *, zs_rocm_attr pos, size_t n, float dx, int side,
                                              int keyIsOrigin, int K, const float *src, float *dst, int C, unsigned *cellMask, int *status);
/* occupied slots in slot order (slots may be NULL: count only); synchronises */
ZS_ROCM_EXPORT size_t zs_rocm_mpm_slot_list(zs_rocm_policy *, const unsigned *cellMask, size_t nbins, int K, int *slots);
/* the slotted storage's buffers in one POD (all device pointers, owned by the caller) */
typedef struct zs_rocm_slot_storage {
  unsigned *cellMask; /* [nbins][64] */
  int K;
  const int *nbr;     /* [nblocks][8]  zs_rocm_mpm_build_neighbors */
  const int *nbr27;   /* [nblocks][27] zs_rocm_mpm_build_neighbors27 */
  int *moverCount;
  unsigned *claim;
  float *moverRec;
  int outboxCap;
  int *status;        /* [ZS_ROCM_SLOT_STATUS_WORDS] */
  const unsigned char *blockEdge; /* [nblocks] from zs_rocm_mpm_partition_edge, or NULL (no early warning in status[3]) */
} zs_rocm_slot_storage;
/* edge[i] = 1 if one of the blocks at offsets [lo, hi]^3 of block i is not in the partition (lo = -1, hi = 2: a particle of a block with
 * edge == 0 can move into any neighbouring block and still scatter its whole stencil) */
ZS_ROCM_EXPORT void zs_rocm_mpm_partition_edge(zs_rocm_policy *, const zs_rocm_bht_3 *, unsigned char *edge /* [nblocks] */, int keyStride,
                                               int lo, int hi);
/* Re-partition of slotted storage in place (r05; no reference counterpart -- the reference never orders particles): the partition a fused time
 * loop runs on has to follow the particles (closed-loop trigger: status word [3]).  (1) the reference's ComputeSparsity
 * (simulation/sparsity/SparsityOp.hpp:65-86) taken from the occupancy words instead of the particle positions -- a particle is stored under the
 * cell of its base node -- into `newTab` (a freshly reset table); enlarge it with zs_rocm_mpm_enlarge_sparsity as usual.  (2) every bin that
 * holds particles moves, as whole tile rows, to the number its block has in `newTab`; `newMask` and (optionally) `newGrid` -- the node
 * velocities the next step gathers from -- are written for the whole new partition.  No particle is read, re-binned or re-slotted:
 * ~4 ms instead of ~50 ms per re-partition of the 64 Mi-particle column.  Buffers: newBuf = nbins(new) * K * 64 * C floats, newMask = nbins(new) * 64 words,
 * newGrid = nblocks(new) * 7 * side^3 floats.  Returns 0 / -1 (bad arguments); status[2] if a populated block is missing from `newTab`.
 * Only the slots that `newMask` selects are written in newBuf: every other row keeps whatever the buffer held (zs_rocm_mpm_slot_particles
 * zero-fills empty slots, this call does not) -- after a re-partition in place "a slot is defined iff its occupancy bit is set" is the
 * storage's invariant; every kernel of the path reads masked slots only. */
ZS_ROCM_EXPORT void zs_rocm_mpm_slot_compute_sparsity(zs_rocm_policy *, const zs_rocm_bht_3 *oldTab, const unsigned *cellMask, size_t nblocksOld,
                                                      int side, int keyIsOrigin, zs_rocm_bht_3 *newTab);
ZS_ROCM_EXPORT int zs_rocm_mpm_reslot(zs_rocm_policy *, const zs_rocm_bht_3 *oldTab, const zs_rocm_bht_3 *newTab, int side, int K, int C,
                                      const float *oldBuf, float *newBuf, const unsigned *oldMask, unsigned *newMask, const float *oldGrid,
                                      float *newGrid, int *status);
/* the step over blocks [blockBegin, blockEnd) on the storage `st` (see zs_rocm_mpm_g2p2g_slotted_range for finish) */
ZS_ROCM_EXPORT int zs_rocm_mpm_g2p2g_slots(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                           const float *gridA, float *gridB, size_t nblocks, const zs_rocm_slot_storage *st, int writeAll,
                                           size_t blockBegin, size_t blockEnd, int finish);
ZS_ROCM_EXPORT int zs_rocm_mpm_g2p2g_slotted(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                             const float *gridA, float *gridB, size_t nblocks, unsigned *cellMask, int K, const int *nbr,
                                             const int *nbr27, int *moverCount, unsigned *claim, float *moverRec, int outboxCap,
                                             int writeAll, int *status);
/* the same over blocks [blockBegin, blockEnd); finish != 0 (ONCE per step, with or after the last range): the step's outbox records get
 * their slots and departures / arrivals enter the occupancy words.  Multi-GPU: boundary blocks first, their ghost sums travel while the
 * interior range computes (zs_rocm_mpm_g2p2g_range is the compact-storage counterpart) */
ZS_ROCM_EXPORT int zs_rocm_mpm_g2p2g_slotted_range(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                                   const float *gridA, float *gridB, size_t nblocks, unsigned *cellMask, int K, const int *nbr,
                                                   const int *nbr27, int *moverCount, unsigned *claim, float *moverRec, int outboxCap,
                                                   int writeAll, int *status, size_t blockBegin, size_t blockEnd, int finish);
/* particles.stress := model(F, logJp) * volume, logJp updated (no-op when particles.stress.base == NULL) */
/* Fused transfer: G2P of step n (from gridA: velocities after zs_rocm_mpm_grid_update) and P2G of step n+1 (into gridB,
 * zeroed by the caller) in one pass over the binned particles -- the reference's G2P2GTransfer idea
 * (simulation/transfer/G2P2G.hpp:20-148).  Same results as zs_rocm_mpm_g2p followed by zs_rocm_mpm_p2g; HBM traffic per
 * particle drops from 296.5 B to 116.5 B because v, C and the cached stress stay on chip.  Requires binned particles and
 * the `stress` attribute (state of the particles that take the exact path is parked there).  writeAll != 0 also writes
 * v, C, stress of every particle (e.g. on the last step).  Returns 0, or -1 if the requirements are not met. */
ZS_ROCM_EXPORT int zs_rocm_mpm_g2p2g(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                     const float *gridA, float *gridB, size_t nblocks, const int *binStart,
                                     const unsigned *cellCount, const int *nbr, int writeAll);
/* The same over blocks [blockBegin, blockEnd) only (multi-GPU step: the blocks near a rank boundary are numbered first and
 * launched first, their ghost sums travel while the interior range computes).  driftFlag (device int[3], may be NULL):
 * [0] is set to 1 when an exact-path particle sits more than one 4^3 bin away from the bin it is stored in (the margin that
 * keeps interior blocks from touching shared blocks no longer holds: re-bin); [1] accumulates the number of particles the
 * call handled on the exact path (moved out of their cell since the last re-bin) -- the caller's re-bin trigger; [2] is set
 * to 1 when a particle's stencil reached a node whose block is not in the partition (the reference does not check,
 * P2G.hpp:109-110; here the contribution is dropped and the caller is told to rebuild the partition). */
ZS_ROCM_EXPORT int zs_rocm_mpm_g2p2g_range(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles, const zs_rocm_bht_3 *,
                                           const float *gridA, float *gridB, size_t nblocks, const int *binStart,
                                           const unsigned *cellCount, const int *nbr, int writeAll, size_t blockBegin,
                                           size_t blockEnd, int *driftFlag);
/* Fused step that re-bins on the fly.  binStart / cellCount describe the NEW binned order (zs_rocm_mpm_bin_particles on the
 * current positions, `order` = its permutation: slot i holds the particle stored at order[i]); the step's inputs m, x, F, logJp
 * are read from slot order[i] of particlesIn, everything the step stores (incl. m) goes to slot i of particlesOut.  Both
 * particle sets must be two buffers of one layout.  The physical re-bin thus costs no pass of its own, and every particle
 * starts the step in the cell it is binned in. */
ZS_ROCM_EXPORT int zs_rocm_mpm_g2p2g_reorder_range(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles particlesOut,
                                                   zs_rocm_particles particlesIn, const int *order, const zs_rocm_bht_3 *,
                                                   const float *gridA, float *gridB, size_t nblocks, const int *binStart,
                                                   const unsigned *cellCount, const int *nbr, int writeAll, size_t blockBegin,
                                                   size_t blockEnd, int *driftFlag);
ZS_ROCM_EXPORT void zs_rocm_mpm_update_stress(zs_rocm_policy *, const zs_rocm_mpm_params *, zs_rocm_particles);
/* channels the library expects behind zs_rocm_particles.stress (6 since r04; 9 before): a caller that allocates the attribute checks this
 * once -- a 9-channel attribute handed to a 6-channel library would be misread silently */
ZS_ROCM_EXPORT int zs_rocm_mpm_stress_channels(void);
/* per-particle constitutive update alone (physics/ConstitutiveModel_Vol_dP.hpp:10-47,246-326):
 * PF[9n] AoS out; F (and logJp) updated in place for plastic models.  Test/diagnostic entry point. */
ZS_ROCM_EXPORT void zs_rocm_mpm_stress(zs_rocm_policy *, const zs_rocm_mpm_params *, float *F, float *logJp, size_t n, float *PF);
ZS_ROCM_EXPORT void zs_rocm_svd3(zs_rocm_policy *, const float *F, size_t n, float *U, float *S, float *V);

/* ghost-block halo exchange helpers for the multi-GPU domain decomposition (no reference counterpart:
 * zpc has no collective layer).  pack: buf[i][c][k] = grid[blocks[i]][chn0+c][k];
 * unpack: add = 0 set, 1 add (every block listed once), 2 atomic add (a block may be listed several times: concatenated
 * messages of several peers). */
/* owner rank of every particle for the block-aligned spatial split of the multi-GPU driver: cell = floor(x / dx) clamped to
 * [lo, hi); axis d is cut into dims[d] slabs at lo + (len k / dims[d]) rounded down to a multiple of `align` cells;
 * rank = (r0 * dims[1] + r1) * dims[2] + r2 */
ZS_ROCM_EXPORT void zs_rocm_mpm_owner_rank(zs_rocm_policy *, zs_rocm_attr pos, size_t n, float dx, const int lo[3], const int hi[3],
                                           const int dims[3], int align, int *owner);
/* counts[r] (device, `world` ints, world <= 1024) = number of entries of owner[0 .. n) equal to r */
ZS_ROCM_EXPORT void zs_rocm_mpm_owner_counts(zs_rocm_policy *, const int *owner, size_t n, int world, int *counts);
ZS_ROCM_EXPORT void zs_rocm_mpm_halo_pack(zs_rocm_policy *, const float *grid, const int *blocks, size_t nb, int side,
                                          int chn0, int nchn, float *buf);
ZS_ROCM_EXPORT void zs_rocm_mpm_halo_unpack(zs_rocm_policy *, float *grid, const int *blocks, size_t nb, int side,
                                            int chn0, int nchn, const float *buf, int add);


/* ======================================================================== (B) multi-GPU exchange steps on RCCL (zpc_amd/csrc/dist.hip)
 * One process per GPU, one communicator per process; the reference has no collective layer, these are the exchange
 * steps the spatially sharded MPM path has: ghost-block halo exchange (grouped ncclSend / ncclRecv over the point-to-point xGMI
 * links), allreduce(max) for the CFL step, counts + uneven all-to-all for particle migration.  All calls enqueue on the policy's
 * stream.  Return 0, or -1 after an RCCL error (also latched in zs_rocm_last_error). */
typedef struct zs_rocm_dist zs_rocm_dist;
ZS_ROCM_EXPORT size_t zs_rocm_dist_unique_id_bytes(void);
ZS_ROCM_EXPORT int zs_rocm_dist_unique_id(void *out); /* rank 0; the launcher distributes the bytes */
ZS_ROCM_EXPORT zs_rocm_dist *zs_rocm_dist_create(int rank, int world, const void *uniqueId, int device);
ZS_ROCM_EXPORT void zs_rocm_dist_destroy(zs_rocm_dist *);
ZS_ROCM_EXPORT int zs_rocm_dist_rank(const zs_rocm_dist *);
ZS_ROCM_EXPORT int zs_rocm_dist_world(const zs_rocm_dist *);
/* ncclCommCount of the communicator (-1: no communicator): zs_rocm_dist_create already fails when it differs from `world` */
ZS_ROCM_EXPORT int zs_rocm_dist_comm_count(const zs_rocm_dist *);
ZS_ROCM_EXPORT int zs_rocm_dist_halo_exchange(zs_rocm_dist *, zs_rocm_policy *, float *grid, int side, int chn0, int nchn, const int *blocks,
                                              size_t totalBlocks, int npeers, const int *peerRank, const size_t *peerOffset,
                                              const size_t *peerCount, float *sendbuf, float *recvbuf);
ZS_ROCM_EXPORT int zs_rocm_dist_allreduce_f32(zs_rocm_dist *, zs_rocm_policy *, float *buf, size_t n, int op); /* 0 sum, 1 max, 2 min */
ZS_ROCM_EXPORT int zs_rocm_dist_allreduce_i64(zs_rocm_dist *, zs_rocm_policy *, long long *buf, size_t n, int op);
ZS_ROCM_EXPORT int zs_rocm_dist_alltoall_i64(zs_rocm_dist *, zs_rocm_policy *, const long long *send, long long *recv);
ZS_ROCM_EXPORT int zs_rocm_dist_alltoallv_f32(zs_rocm_dist *, zs_rocm_policy *, const float *send, const size_t *sendCounts,
                                              const size_t *sendOffsets, float *recv, const size_t *recvCounts, const size_t *recvOffsets);
ZS_ROCM_EXPORT int zs_rocm_dist_barrier(zs_rocm_dist *, zs_rocm_policy *);
/* The halo plan: which of this rank's grid blocks do other ranks hold as well (set at partition-build time).  _from_keys is the pure host
 * part (callable without a GPU): keysAll = the ranks' key lists back to back (counts[r] keys of 3 ints, each list in its rank's block-number
 * order); per peer that shares blocks with `rank`, in rank order: the shared keys in lexicographic order as positions in this rank's list
 * (both sides of a pair derive the same order).  peerRank / peerOffset / peerCount: capacity world - 1; blocks: capacity = the return value
 * (call with NULL outputs to size).  _create is collective: RCCL all-gather of the key lists (keys = the partition's activeKeys, device),
 * plan on the host, exchange buffers allocated; _exchange = zs_rocm_dist_halo_exchange over the plan's lists and buffers. */
typedef struct zs_rocm_halo_plan zs_rocm_halo_plan;
ZS_ROCM_EXPORT size_t zs_rocm_halo_plan_from_keys(const int *keysAll, const size_t *counts, int world, int rank, int *npeers, int *peerRank,
                                                  size_t *peerOffset, size_t *peerCount, int *blocks);
ZS_ROCM_EXPORT zs_rocm_halo_plan *zs_rocm_dist_halo_plan_create(zs_rocm_dist *, zs_rocm_policy *, const int *keys, size_t nblocks, int side);
ZS_ROCM_EXPORT void zs_rocm_dist_halo_plan_destroy(zs_rocm_halo_plan *);
ZS_ROCM_EXPORT int zs_rocm_dist_halo_plan_npeers(const zs_rocm_halo_plan *);
ZS_ROCM_EXPORT size_t zs_rocm_dist_halo_plan_blocks(const zs_rocm_halo_plan *);
ZS_ROCM_EXPORT size_t zs_rocm_dist_halo_plan_bytes(const zs_rocm_halo_plan *);   /* bytes sent (= received) per exchange of all 7 channels */
ZS_ROCM_EXPORT const int *zs_rocm_dist_halo_plan_block_list(const zs_rocm_halo_plan *);   /* device */
ZS_ROCM_EXPORT int zs_rocm_dist_halo_plan_exchange(zs_rocm_halo_plan *, zs_rocm_dist *, zs_rocm_policy *, float *grid, int chn0, int nchn);
/* a plan from explicit lists (host arrays): slice k of blocks[total] = local block numbers shared with rank peerRank[k] */
ZS_ROCM_EXPORT zs_rocm_halo_plan *zs_rocm_dist_halo_plan_from_lists(zs_rocm_dist *, int side, int npeers, const int *peerRank,
                                                                    const size_t *peerOffset, const size_t *peerCount, const int *blocks,
                                                                    size_t total);
/* One sub-step of the slotted MPM path in ONE call (zpc_amd/csrc/dist.hip): gridB := 0 (unless gridBIsClear, below); fused G2P (gridA) + P2G (gridB) over the boundary
 * blocks [0, nBoundary), then the interior blocks (+ re-home / commit); the ghost-block exchange of the plan on commPolicy's stream behind
 * the boundary range, overlapping the interior (rangeSchedule: as two launches, or as one whose boundary workgroups count themselves off);
 * grid update of gridB (extf, maxVelSqr) [+ collider]; allreduce(max) of maxVelSqr.  Nothing
 * of the caller runs between the kernels.  dist / plan / commPolicy / maxVelSqr / collider / haloGrid may be NULL (single rank: no exchange).
 * haloGrid: the grid whose shared blocks are exchanged (NULL: gridB).  The reference's building blocks for such a schedule are
 * pol.device(i) / .stream(i) / .listen() (cuda/execution/ExecutionPolicy.cuh:364-399).
 * A non-zero return is FATAL for the object being stepped: when the exchange fails in the overlapped schedule the particle side of the step
 * has still been committed (both ranges ran, re-home and commit included, so that the slot storage stays consistent) but gridB has neither
 * been completed nor updated -- the particles are one step ahead of the grids.  Do not retry the step (it would advance the particles
 * twice) and do not continue from this state. */
typedef struct zs_rocm_mpm_step {
  const zs_rocm_mpm_params *params;
  zs_rocm_particles particles;
  const zs_rocm_bht_3 *table;
  const float *gridA;
  float *gridB;
  size_t nblocks;
  const zs_rocm_slot_storage *storage;
  int writeAll;
  float extf[3];
  float *maxVelSqr;
  const zs_rocm_collider *collider;
  size_t nBoundary;
  zs_rocm_dist *dist;
  zs_rocm_halo_plan *plan;
  zs_rocm_policy *commPolicy;
  float *haloGrid;
  void *evTransferBegin, *evTransferEnd; /* hipEvent_t or NULL: recorded on the policy's stream around the transfer kernels (timing) */
  void **evBreakdown;                    /* NULL, or ZS_ROCM_STEP_EVENTS hipEvent_t (timing enabled, created on the policy's device) recorded along
                                            the step -- on the policy's stream: [0] start, [1] boundary range done, [2] interior range + re-home +
                                            commit done, [5] exchange waited for, [6] grid update done, [7] CFL allreduce done; on commPolicy's
                                            stream: [3] exchange started, [4] exchange done (without overlap [3], [4] are recorded on the policy's
                                            stream around the exchange and [1] == [0]).  A rank's step time splits into
                                            boundary [0,1], interior [1,2], waiting for the exchange [2,5], grid update [5,6], allreduce [6,7];
                                            the exchange itself is [3,4] */
  int haloChannels;                      /* grid channels [0, haloChannels) of the shared blocks are exchanged; 0 = all 7.  4 = {m, mv}: all a step
                                            ever reads of a ghost block -- the grid update forms v = mv / m + extf dt and G2P gathers v, exactly as
                                            ComputeGridBlockVelocity / G2PTransfer of the reference do (simulation/grid/GridOp.hpp:90-104); the rhs
                                            channels 4..6 of a shared block then keep this rank's partial sums */
  int rangeSchedule;                     /* overlapped schedule only (commPolicy set, 0 < nBoundary < nblocks): how the boundary blocks' sums get to
                                            the exchange stream early.
                                            ZS_ROCM_RANGES_IN_TURN (0): two launches on the policy's stream, boundary range then interior range.
                                            ZS_ROCM_RANGES_SIDE_BY_SIDE (1): the boundary range on commPolicy's stream (give it the higher
                                            priority) in front of the exchange, the interior range on the policy's stream at the same time; re-home /
                                            commit wait for both.  The interior's workgroups fill the CUs the boundary range's last workgroups
                                            leave idle, but the two launches share the CUs: the boundary range ends later than it would alone.
                                            ZS_ROCM_RANGES_ONE_LAUNCH (2; 8^3 blocks): ONE launch over all blocks -- workgroups are dispatched in
                                            block order, the boundary blocks come first -- whose boundary workgroups count themselves off on a
                                            device word; a one-wave gate kernel on commPolicy's stream waits for the count and the exchange runs
                                            behind it.  No launch boundary inside the step: no tail, no sharing.
                                            evBreakdown[1] (boundary done) is recorded on commPolicy's stream for 1 and 2; [0,1] and [0,2] overlap. */
  float *handoverSnapshot;               /* NULL, or (test hook, overlapped schedule) plan-blocks x side^3 floats: the MASS channel of gridB's shared blocks, packed like the
                                            exchange buffer (zs_rocm_mpm_halo_pack, chn0 = 0, nchn = 1) on commPolicy's stream at the moment the exchange starts.  Only the
                                            boundary blocks write those nodes, so it must equal the same pack taken after the step: the check that the hand-over of a
                                            schedule lets the exchange see complete sums (tests/test_dist_gpu.py) */
  float *gridClear;                      /* NULL, or (8^3 blocks; ignored for 4^3) a THIRD grid of the same partition, 16-byte aligned, neither gridA nor
                                            gridB (else -1): the fused block kernel writes zero over it, every workgroup its own block, every block of
                                            [0, nblocks) once per step whatever the range schedule.  Rotate three grids -- gather from A, scatter into B,
                                            clear C; next step gather from B, scatter into C, clear A -- and the grid that becomes the target has been
                                            cleared by the step before */
  int gridBIsClear;                      /* non-zero: gridB is all zero already (the previous step's gridClear, same partition, nothing written to it
                                            since), the call skips its memset of gridB.  Honoured only with gridClear != NULL and 8^3 blocks; in every
                                            other case gridB is cleared here as before.  Say 0 after anything that re-partitions or writes the grids */
  const zs_rocm_levelset *levelset;      /* NULL, or the boundary is this level set with `collider`'s type and motion (zs_rocm_mpm_apply_boundary_levelset);
                                            a level set without a collider is refused (-1) before anything runs */
} zs_rocm_mpm_step;
#define ZS_ROCM_STEP_EVENTS 8
#define ZS_ROCM_RANGES_IN_TURN 0
#define ZS_ROCM_RANGES_SIDE_BY_SIDE 1
#define ZS_ROCM_RANGES_ONE_LAUNCH 2
ZS_ROCM_EXPORT int zs_rocm_mpm_step_slotted(zs_rocm_policy *, const zs_rocm_mpm_step *);

#ifdef __cplusplus
}
#endif
#endif /* ZS_ROCM_H */
