// joblist.h -- the job list of a launch that serves several codewords, in a pinned image the kernel reads itself: the jobs (J: the kernel's job struct),
// then tile_job[workgroup] = the job that workgroup works on.  A codeword's workgroups (modem::tiles_of) are consecutive; its job records the first of them.
#pragma once
#include "modem_device.h"
#include "stage.h"

namespace phyhip {

struct JobListLayout {
  size_t o_jobs, o_tj, end; // byte offsets in the image: the jobs, the tile table, the first byte behind both
};
inline JobListLayout job_list_layout(size_t at, size_t job_bytes, size_t n_tiles)
{
  const size_t o_tj = al256(at + job_bytes);
  return {at, o_tj, al256(o_tj + n_tiles * sizeof(uint32_t))};
}

template <class J>
struct JobList {
  J* const        jobs;
  uint32_t* const tile_job;
  uint32_t        n_tiles = 0; // listed so far
  JobList(uint8_t* image, size_t o_jobs, size_t o_tj) : jobs(reinterpret_cast<J*>(image + o_jobs)), tile_job(reinterpret_cast<uint32_t*>(image + o_tj)) {}
  uint32_t append(uint32_t k, uint32_t cnt) // job k covers the next cnt workgroups; returns the first of them (the job's tile0)
  {
    const uint32_t tile0 = n_tiles;
    for (uint32_t t = 0; t < cnt; t++) {
      tile_job[n_tiles++] = k;
    }
    return tile0;
  }
};

} // namespace phyhip
