// The shared pieces of the multi-tensor launches (csrc/adam.hip, csrc/gradnorm.hip): one workgroup of 256 threads per entry of a
// block map, blockmap[b] = {tensor index into a pointer table, chunk index within that tensor}.
#pragma once

struct AdamEntry {                     // a row of optim.Adam's pointer table: 5 x 8 bytes
  float* p; const float* g; float* m; float* v; long long n;
};

struct CopyEntry {                     // a row of cy_multi_copy's table: {tensor, offset into flat, numel}
  float* t; long long off; long long n;
};

// [begin, end) of the elements that block-map entry bm covers in a tensor of numel elements
__device__ __forceinline__ void chunk_range(int2 bm, int chunk, long long numel, long long& begin, long long& end) {
  begin = (long long)bm.y * chunk;
  end = begin + chunk;
  if (end > numel) end = numel;
}
