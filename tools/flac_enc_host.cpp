// flac_enc_host.cpp — the FLAC encode kernels (csrc/flac_enc.hip) compiled for the host: 64
// threads and real barriers stand in for the wave, so that AddressSanitizer and UBSan see every
// load, store and shift before the kernels first run on a device.  Never run on a GPU machine
// and not wired into pytest; tools/flac_enc_host_check.py drives it over the test matrix.
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I nightcore-to-flac-analyzer_amd/csrc tools/flac_enc_host.cpp -lpthread -o /tmp/flac_enc_host
//   /tmp/flac_enc_host cases.bin out.bin [fuzz_rounds seed]
//
// cases.bin: int64 n_cases, then per case int64[8] = channels, bits, rate, total, block, level,
// is_float, 0 and the planar samples (int32 or float32, channels x total).  out.bin: per case
// int64 n_frames, int64 n_bytes, the packed frames, int32 frame_bytes / records[25] / clipped /
// status per frame, and the int32 work buffer (channels x total).  With fuzz_rounds, every case is
// also run that many times with one to three table cells overwritten by random values (and the
// result packed); the statuses are counted, nothing else is checked: the sanitizers are the check.
#include <math.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#define NC_FLAC_HOST_SIM 1
#define __device__
#define __global__
#define __shared__ static
#define __launch_bounds__(n)
#define NC_COHERENT_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)

struct Idx {
  int x;
};
static thread_local Idx threadIdx, blockIdx;
static pthread_barrier_t g_bar;
static uint64_t g_xch[2][64];
static thread_local int g_turn;

static inline void __syncthreads() { pthread_barrier_wait(&g_bar); }
static inline void __threadfence() { __atomic_thread_fence(__ATOMIC_SEQ_CST); }
// one barrier per exchange: the buffers alternate, and a lane writes buffer p again only after
// the barrier of the exchange in between, which every lane reaches after its read of p
template <class T>
static inline T lane_exchange(T v, int src) {
  static_assert(sizeof(T) <= 8, "32- and 64-bit shuffles only");
  uint64_t bits = 0;
  memcpy(&bits, &v, sizeof(T));
  uint64_t* buf = g_xch[g_turn];
  g_turn ^= 1;
  buf[threadIdx.x] = bits;
  pthread_barrier_wait(&g_bar);
  bits = buf[src >= 0 && src < 64 ? src : threadIdx.x];
  memcpy(&v, &bits, sizeof(T));
  return v;
}
template <class T>
static inline T __shfl_xor(T v, int d, int) { return lane_exchange(v, threadIdx.x ^ d); }
template <class T>
static inline T __shfl_up(T v, int d, int) { return lane_exchange(v, threadIdx.x - d); }
template <class T>
static inline T __shfl_down(T v, int d, int) { return lane_exchange(v, threadIdx.x + d); }
static inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }

#include "flac_enc.hip"

namespace {

struct Job {
  const int* pcm_in;
  const float* f32_in;
  int* pcm_q;
  int64_t in_len;
  const int64_t* frames;
  int64_t n_frames;
  const int64_t* files;
  int n_files, level;
  uint32_t* slots;
  int64_t slot_bytes;
  int *frame_bytes, *records, *clipped, *status;
  const int64_t* offsets;
  uint32_t* out;
  int64_t out_bytes;
  bool pack;
};
Job g_job;

void* lane_main(void* arg) {
  threadIdx.x = (int)(intptr_t)arg;
  const Job& j = g_job;
  for (int64_t fr = 0; fr < j.n_frames; ++fr) {
    blockIdx.x = (int)fr;
    if (j.pack)
      nc::flac_pack_kernel(j.slots, j.slot_bytes, j.frames, j.n_frames, j.frame_bytes, j.offsets, j.out, j.out_bytes);
    else
      nc::flac_encode_kernel(j.pcm_in, j.f32_in, j.pcm_q, j.in_len, j.frames, j.n_frames, j.files, j.n_files, j.level,
                             j.slots, j.slot_bytes, j.frame_bytes, j.records, j.clipped, j.status);
    pthread_barrier_wait(&g_bar);  // the statics standing in for LDS belong to one frame at a time
  }
  return nullptr;
}

void launch() {
  pthread_t th[64];
  for (int i = 0; i < 64; ++i) pthread_create(&th[i], nullptr, lane_main, (void*)(intptr_t)i);
  for (int i = 0; i < 64; ++i) pthread_join(th[i], nullptr);
}

template <class T>
T* exact(size_t n) {  // a heap block of exactly n elements: the sanitizer's red zones sit at both ends
  T* p = (T*)malloc(n * sizeof(T) ? n * sizeof(T) : 1);
  memset(p, 0, n * sizeof(T));
  return p;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* fi = fopen(argv[1], "rb");
  FILE* fo = fopen(argv[2], "wb");
  if (!fi || !fo) return 2;
  const int fuzz = argc > 3 ? atoi(argv[3]) : 0;
  std::mt19937_64 rng(argc > 4 ? atoll(argv[4]) : 1);
  pthread_barrier_init(&g_bar, nullptr, 64);
  int64_t n_cases = 0;
  if (fread(&n_cases, 8, 1, fi) != 1) return 2;
  long fuzz_runs = 0, fuzz_bad = 0;
  for (int64_t ci = 0; ci < n_cases; ++ci) {
    int64_t h[8];
    if (fread(h, 8, 8, fi) != 8) return 2;
    const int64_t nch = h[0], bits = h[1], rate = h[2], total = h[3], block = h[4], level = h[5], is_float = h[6];
    const int64_t n_samples = nch * total;
    int* in = exact<int>(n_samples);
    if (fread(in, 4, n_samples, fi) != (size_t)n_samples) return 2;
    int* q = exact<int>(n_samples);
    const int64_t n_frames = (total + block - 1) / block;
    const uint32_t need = nc::slot_need((int)nch, (int)block, (int)bits);
    int64_t* files = exact<int64_t>(8);
    int64_t* frames = exact<int64_t>(8 * n_frames);
    const int64_t file_row[8] = {0, total, nch, bits, rate, total, 0, 0};
    memcpy(files, file_row, sizeof file_row);
    for (int64_t f = 0; f < n_frames; ++f) {
      const int64_t b = total - f * block < block ? total - f * block : block;
      const int64_t r[8] = {0, f * block, b, f, f * (int64_t)need, 0, 0, 0};
      memcpy(frames + 8 * f, r, sizeof r);
    }
    const int64_t slot_bytes = n_frames * (int64_t)need;
    uint32_t* slots = exact<uint32_t>(slot_bytes / 4);
    int* frame_bytes = exact<int>(n_frames);
    int* records = exact<int>(25 * n_frames);
    int* clipped = exact<int>(n_frames);
    int* status = exact<int>(n_frames);
    int64_t* offsets = exact<int64_t>(n_frames);
    auto run = [&](const int64_t* fr_tab, const int64_t* fl_tab, uint32_t** out, int64_t* out_bytes) {
      memset(slots, 0xA5, slot_bytes);  // the kernel zeroes what it ORs into
      g_job = Job{is_float ? nullptr : in, is_float ? (const float*)in : nullptr, q, n_samples, fr_tab, n_frames,
                  fl_tab, 1, (int)level, slots, slot_bytes, frame_bytes, records, clipped, status, offsets, nullptr, 0,
                  false};
      launch();
      int64_t sum = 0;
      for (int64_t f = 0; f < n_frames; ++f) {
        offsets[f] = sum;
        sum += frame_bytes[f];
      }
      *out_bytes = (sum + 3) & ~INT64_C(3);
      *out = exact<uint32_t>(*out_bytes / 4);
      g_job.pack = true;
      g_job.out = *out;
      g_job.out_bytes = *out_bytes;
      launch();
      return sum;
    };
    uint32_t* out = nullptr;
    int64_t out_bytes = 0;
    const int64_t n_bytes = run(frames, files, &out, &out_bytes);
    fwrite(&n_frames, 8, 1, fo);
    fwrite(&n_bytes, 8, 1, fo);
    fwrite(out, 1, n_bytes, fo);
    fwrite(frame_bytes, 4, n_frames, fo);
    fwrite(records, 4, 25 * n_frames, fo);
    fwrite(clipped, 4, n_frames, fo);
    fwrite(status, 4, n_frames, fo);
    fwrite(q, 4, n_samples, fo);
    free(out);
    for (int r = 0; r < fuzz; ++r) {
      int64_t* fr2 = exact<int64_t>(8 * n_frames);
      int64_t* fl2 = exact<int64_t>(8);
      memcpy(fr2, frames, 64 * n_frames);
      memcpy(fl2, files, 64);
      const int hits = 1 + (int)(rng() % 3);
      for (int k = 0; k < hits; ++k) {
        const int64_t pool[] = {-1, 0, 1, 3, 15, 17, 25, 64, 65535, 16385, INT64_C(1) << 31, INT64_C(1) << 40,
                                INT64_MAX, INT64_MIN, (int64_t)(rng() % 100000), -(int64_t)(rng() % 100000),
                                (int64_t)rng()};
        const int64_t v = pool[rng() % (sizeof pool / sizeof pool[0])];
        if (rng() % 3 == 0) fl2[rng() % 6] = v;
        else fr2[8 * (rng() % n_frames) + rng() % 5] = v;
      }
      uint32_t* o2 = nullptr;
      int64_t ob2 = 0;
      run(fr2, fl2, &o2, &ob2);
      ++fuzz_runs;
      for (int64_t f = 0; f < n_frames; ++f) fuzz_bad += status[f] != 0;
      free(o2);
      free(fr2);
      free(fl2);
    }
    free(in), free(q), free(files), free(frames), free(slots), free(frame_bytes), free(records), free(clipped),
        free(status), free(offsets);
  }
  fclose(fi);
  fclose(fo);
  printf("%lld cases; %ld corrupted runs, %ld frame statuses\n", (long long)n_cases, fuzz_runs, fuzz_bad);
  return 0;
}
