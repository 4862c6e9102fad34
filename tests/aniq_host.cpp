// The library's rule for character states and animation queues (clap_amd/csrc/aniq_dev.h), compiled for the host: the
// same two functions the kernels of aniq.hip call once per lane, called once per character over host arrays.
// tests/test_aniq.py builds this with g++ and holds it to tests/aniqref.py where no GPU is at hand.
#include "aniq_dev.h"

extern "C" void aniq_host_state(const clapgpu_aniq *q, uint32_t n_movers, const uint8_t *request, const float *motion, double now)
{
    for (uint32_t c = 0; c < q->n; c++) aniq::state_step(*q, c, n_movers, request, motion, now);
}

extern "C" void aniq_host_time(const clapgpu_aniq *q, double now)
{
    for (uint32_t c = 0; c < q->n; c++) aniq::time_step(*q, c, now);
}
