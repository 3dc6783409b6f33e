// pathseq_stream_check.cpp -- TEST-ONLY, stand-alone: a main of its own over the host build of the path-sequence program, so that it can
// be built with -fsanitize=address,undefined and run as it is (tests/emul/pathseq.mk, target `check`; nothing is loaded into another
// program).  It reads the file tests/pathseq_stream_dump.py writes -- the fabricated streams of tests/test_pathseq.py with the bytes the
// model expects -- and puts each through the hook of ga_emul_pathseq.cpp: the moves in a buffer of exactly their size, the bytes in a
// heap buffer of exactly the expected size, so that a load or a store outside either is the sanitizer's to report; then once more
// into a buffer one byte short, which the hook must refuse without writing.
// Exit status 0 and a line of totals when everything agrees.
#include <cstdio>
#include <fstream>
#include <string>

#include "ga_emul_pathseq.cpp"

namespace {
int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; fprintf(stderr, "line %d: ", __LINE__); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); } } while (0)
}  // namespace

int main(int argc, char** argv)
{
	if (argc != 2) { fprintf(stderr, "usage: %s FILE (written by tests/pathseq_stream_dump.py)\n", argv[0]); return 2; }
	std::ifstream in(argv[1]);
	if (!in) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
	size_t streams = 0;
	unsigned long long bases = 0;
	std::string tag;
	while (in >> tag)
	{
		if (tag != "P") { CHECK(false, "unknown line %s", tag.c_str()); break; }
		uint32_t nNodes, nodeLen, startRow, traceRows, nMoves;
		int backward;
		std::string hex, want;
		in >> nNodes >> nodeLen >> startRow >> traceRows >> backward >> nMoves >> hex >> want;
		if (want == "-") want.clear();
		std::vector<uint8_t> moves(nMoves);
		for (uint32_t k = 0; k < nMoves && 2 * k + 1 < hex.size(); k++) moves[k] = (uint8_t)std::stoul(hex.substr(2 * k, 2), nullptr, 16);
		std::vector<uint8_t> got(want.size(), 0xA5);
		const long n = ga_emul_pathseq_stream(moves.data(), nMoves, nNodes, nodeLen, startRow, traceRows, backward, got.data(), got.size());
		CHECK(n == (long)want.size(), "stream %zu: %ld bases, expected %zu", streams, n, want.size());
		CHECK(n != (long)want.size() || std::equal(want.begin(), want.end(), got.begin()), "stream %zu: bases differ", streams);
		if (!want.empty())
		{
			std::vector<uint8_t> tight(want.size() - 1, 0xA5);
			CHECK(ga_emul_pathseq_stream(moves.data(), nMoves, nNodes, nodeLen, startRow, traceRows, backward, tight.data(), tight.size()) == -1, "stream %zu: a place one byte short accepted", streams);
			for (uint8_t b : tight) CHECK(b == 0xA5, "stream %zu: a refused call wrote", streams);
		}
		streams++;
		bases += (unsigned long long)(n > 0 ? n : 0);
	}
	printf("%zu streams, %llu bases written, %d failures\n", streams, bases, failures);
	return failures || !streams ? 1 : 0;
}
