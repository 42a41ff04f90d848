// The passes of goldrush-path over its input, in the order gr_path.cpp runs them: -1 to continue, else the exit code.
#pragma once
#include "gr_classifier.hpp"
#include "gr_writer.hpp"

namespace gr {

int calc_ntcard_genome_size(PathRun& run, uint64_t& genome_size); // --ntcard
int calc_min_phred_threshold(PathRun& run);                       // -P 0
int fill_bit_vector(PathRun& run, Resident& res);
struct FillCounts
{
  size_t num_reads = 0, num_passed_reads = 0, by_phred = 0, by_delta = 0, by_length = 0, by_bases = 0;
};
int say_fill_counts(const PathRun& run, const FillCounts& n); // (gr_golden.cpp fills from what the first stage kept)
// the classification pass: over the batches the fill pass left on the device, or over the input read once more
int classify_resident(PathRun& run, Resident& res, Classifier& cls, SinkState& sink);
int classify_source(PathRun& run, Classifier& cls, SinkState& sink);
// an input that could not be read to its end is an error, not a shorter input (gr_fastq.hpp): says so; asked behind every pass
bool input_error();
// behind a pass that returned ec: the lines of its aligned BAM files, then its exit code, or 1 for an input error
int after_pass(PathRun& run, int ec);

} // namespace gr
